// lcv_wire_layout.hpp — the SSZ wire layout of the light-client containers, described once: the device encoder
// (lcv_wire_enc.hpp), the device decoder (lcv_wire_dec.hpp), the host decoder (lcv_wire.cpp) and the driver take
// every field, size and check from here.  Containers: sync-protocol.md:96-101 LightClientHeader, :109-115
// LightClientBootstrap, :120-133 LightClientUpdate, :138-148 FinalityUpdate, :153-160 OptimisticUpdate; fixed parts in
// field order, a 4-byte little-endian offset for every variable-size field (each Deneb / Capella LightClientHeader,
// because its ExecutionPayloadHeader ends in extra_data: ByteList[32]).  Altair-format messages (ALTAIR .. BELLATRIX
// fork versions) have LightClientHeader = {beacon}: every container is fixed-size and a header is its 112 bytes.
//
// Plain C++ over <stdint.h>: the constexpr functions serve host and device alike; the walkers and the acceptance rule
// are LCV_FN where lcv_common.hpp came first (device code, the host simulation) and inline otherwise (g++).
#pragma once
#include <stdint.h>

#if defined(LCV_FN)
#define LCV_WIRE_FN LCV_FN
#define LCV_WIRE_UNROLL LCV_UNROLL
#elif defined(__HIPCC__)
#error "lcv_wire_layout.hpp: a HIP unit includes lcv_common.hpp first (the walkers are device functions there)"
#else
#define LCV_WIRE_FN inline
#define LCV_WIRE_UNROLL
#endif

namespace lcv {

// the packed columns of include/lcv.h.  (K_EXEC_BLOOM_OFF and K_EXEC_EXTRALEN_OFF are places of the 832-byte record
// that the wire format does not know: lcv_ssz.hpp hashes from them)
enum {
  K_BEACON = 112, K_EXEC = 832, K_EXEC_BLOOM_OFF = 544, K_EXEC_EXTRALEN_OFF = 800,
  K_EXEC_BRANCH = 128, K_NSC_BRANCH = 160, K_FIN_BRANCH = 192, K_SC = 24624, K_BITS = 64, K_SIG = 96,
};

// ---- message kinds and fork families (the codes of include/lcv.h).  The bootstrap is a kind of the tables only
enum { WIRE_UPDATE = 0, WIRE_FINALITY = 1, WIRE_OPTIMISTIC = 2, WIRE_BOOTSTRAP = 3, WIRE_DENEB = 0, WIRE_CAPELLA = 1, WIRE_ALTAIR = 2 };
constexpr bool wire_kind_ok(int64_t kind) { return kind >= WIRE_UPDATE && kind <= WIRE_OPTIMISTIC; }
constexpr bool wire_fork_ok(int64_t fork) { return fork >= WIRE_DENEB && fork <= WIRE_ALTAIR; }

// ---- ExecutionPayloadHeader in wire order as (offset in the 832-byte record, length, what): a field of every fork,
// a Deneb field, or the variable-size field, which has its 4-byte offset in the fixed part, its bytes behind it and
// its limit as the length
enum { WX_ALL = 0, WX_DENEB = 1, WX_VAR = 2 };
struct WireExecSeg { uint16_t rec, len; uint8_t what; };
constexpr WireExecSeg kWireExec[] = {
    {0, 32, WX_ALL},                  // parent_hash
    {32, 20, WX_ALL},                 // fee_recipient
    {64, 64, WX_ALL},                 // state_root, receipts_root
    {K_EXEC_BLOOM_OFF, 256, WX_ALL},  // logs_bloom
    {160, 32, WX_ALL},                // prev_randao
    {192, 8, WX_ALL},                 // block_number
    {224, 8, WX_ALL},                 // gas_limit
    {256, 8, WX_ALL},                 // gas_used
    {288, 8, WX_ALL},                 // timestamp
    {320, 32, WX_VAR},                // extra_data: ByteList[32]
    {352, 128, WX_ALL},               // base_fee_per_gas (uint256 LE), block_hash, transactions_root, withdrawals_root
    {480, 8, WX_DENEB},               // blob_gas_used
    {512, 8, WX_DENEB},               // excess_blob_gas
};
enum { WIRE_EXEC_SEGS = sizeof(kWireExec) / sizeof(kWireExec[0]) };
constexpr uint32_t wire_exec_var() {  // the table's row of extra_data
  uint32_t k = 0;
  while (kWireExec[k].what != WX_VAR) ++k;
  return k;
}
enum { K_EXEC_EXTRA_OFF = kWireExec[wire_exec_var()].rec, K_MAX_EXTRA = kWireExec[wire_exec_var()].len };
constexpr uint32_t wire_exec_bytes(uint32_t from, uint32_t to, bool deneb) {  // of the fixed part
  uint32_t s = 0;
  for (uint32_t k = from; k < to; ++k)
    if (kWireExec[k].what != WX_DENEB || deneb) s += kWireExec[k].what == WX_VAR ? 4u : kWireExec[k].len;
  return s;
}
constexpr uint32_t wire_exec_offset_pos() { return wire_exec_bytes(0, wire_exec_var(), true); }
constexpr uint32_t wire_exec_fixed(bool deneb) { return wire_exec_bytes(0, WIRE_EXEC_SEGS, deneb); }

// ---- LightClientHeader (Deneb / Capella): beacon | offset of execution | execution_branch | execution.  The parts
// of a header's columns (lcv_header_cols); a column that is no header has the one part 0
enum { WH_BEACON = 0, WH_EXEC = 1, WH_BRANCH = 2, WH_PARTS = 3 };
constexpr uint32_t wire_header_offset_pos() { return K_BEACON; }
constexpr uint32_t wire_header_fixed() { return K_BEACON + 4u + K_EXEC_BRANCH; }
constexpr uint32_t wire_header_max(bool deneb) { return wire_header_fixed() + wire_exec_fixed(deneb) + K_MAX_EXTRA; }

// ---- the fixed part of every message, both families: the pieces in wire order, each with the batch column it
// belongs to and the kinds that carry it.  A header's piece is its offset field (Deneb / Capella: the headers follow
// the fixed part, attested first) or its beacon header in place (Altair)
enum { WC_ATT = 0, WC_COMMITTEE, WC_NSC_BRANCH, WC_FIN, WC_FIN_BRANCH, WC_BITS, WC_SIG, WC_SLOT, WC_COLS };
struct WirePiece { uint8_t col; uint16_t len; uint8_t kinds; };  // len 0: a header; kinds: bit k = kind k has it
constexpr WirePiece kWirePieces[] = {
    {WC_ATT, 0, 0xF},                   // attested_header (bootstrap: header)
    {WC_COMMITTEE, K_SC, 0x9},          // next_sync_committee (bootstrap: current_sync_committee)
    {WC_NSC_BRANCH, K_NSC_BRANCH, 0x9}, // next_sync_committee_branch (bootstrap: current_sync_committee_branch)
    {WC_FIN, 0, 0x3},                   // finalized_header
    {WC_FIN_BRANCH, K_FIN_BRANCH, 0x3}, // finality_branch
    {WC_BITS, K_BITS, 0x7},             // sync_aggregate.sync_committee_bits
    {WC_SIG, K_SIG, 0x7},               // sync_aggregate.sync_committee_signature
    {WC_SLOT, 8, 0x7},                  // signature_slot
};
enum { WIRE_PIECES = sizeof(kWirePieces) / sizeof(kWirePieces[0]) };
constexpr uint32_t wire_piece_len(uint32_t k, bool altair) {
  return kWirePieces[k].len ? kWirePieces[k].len : altair ? (uint32_t)K_BEACON : 4u;
}
constexpr bool wire_has(uint32_t col, uint32_t kind) {
  for (uint32_t k = 0; k < WIRE_PIECES; ++k)
    if (kWirePieces[k].col == col) return (kWirePieces[k].kinds >> kind) & 1u;
  return false;
}
// where column `col`'s piece starts in a message (col = WC_COLS: the fixed size)
constexpr uint32_t wire_piece_pos(uint32_t col, uint32_t kind, bool altair) {
  uint32_t o = 0;
  for (uint32_t k = 0; k < WIRE_PIECES && kWirePieces[k].col != col; ++k)
    if ((kWirePieces[k].kinds >> kind) & 1u) o += wire_piece_len(k, altair);
  return o;
}
constexpr uint32_t wire_msg_fixed(uint32_t kind, bool altair) { return wire_piece_pos(WC_COLS, kind, altair); }
constexpr uint32_t wire_committee_off(bool altair) { return wire_piece_pos(WC_COMMITTEE, WIRE_UPDATE, altair); }
constexpr uint32_t wire_msg_max(uint32_t kind, uint32_t fork) {
  return fork == WIRE_ALTAIR ? wire_msg_fixed(kind, true)
                             : wire_msg_fixed(kind, false) + (wire_has(WC_FIN, kind) ? 2u : 1u) * wire_header_max(fork == WIRE_DENEB);
}
// the encoder's area per message: the longest message of the kind, rounded up to 16 bytes
constexpr uint32_t wire_encode_pitch(uint32_t kind) {
  const uint32_t d = wire_msg_max(kind, WIRE_DENEB), a = wire_msg_max(kind, WIRE_ALTAIR);
  return ((d > a ? d : a) + 15u) & ~15u;
}
// the kernels' LDS image: the longest message without its committee and the zero fill of its last 16-byte word
constexpr uint32_t wire_image_bytes() { return (wire_msg_max(WIRE_UPDATE, WIRE_DENEB) - K_SC + 16u + 15u) & ~15u; }

static_assert(wire_exec_fixed(true) == 584 && wire_exec_fixed(false) == 568 && wire_exec_offset_pos() == 436, "ExecutionPayloadHeader");
static_assert(wire_header_fixed() == 244 && wire_msg_fixed(WIRE_UPDATE, false) == 528 + K_SC &&
              wire_msg_fixed(WIRE_FINALITY, false) == 368 && wire_msg_fixed(WIRE_OPTIMISTIC, false) == 172, "fixed parts");
static_assert(wire_encode_pitch(WIRE_UPDATE) == 26880 && wire_image_bytes() == 2272, "the update's area and image");

// ---- the walkers: seg(col, part, rec, o, len) for the bytes [o, o + len) of the message that belong at offset
// `rec` of part `part` of column `col`, put(o, v) for an offset field of value v at o; the end is returned.
// A LightClientHeader of column `col` at o, with elen bytes of extra_data:
template <class Seg, class Put>
LCV_WIRE_FN uint32_t wire_walk_header(uint32_t col, uint32_t o, bool deneb, uint32_t elen, Seg seg, Put put) {
  seg(col, WH_BEACON, 0u, o, K_BEACON), o += K_BEACON;
  put(o, wire_header_fixed()), o += 4u;
  seg(col, WH_BRANCH, 0u, o, K_EXEC_BRANCH), o += K_EXEC_BRANCH;
  LCV_WIRE_UNROLL for (uint32_t k = 0; k < WIRE_EXEC_SEGS; ++k) {
    if (kWireExec[k].what == WX_VAR) put(o, wire_exec_fixed(deneb)), o += 4u;
    else if (kWireExec[k].what != WX_DENEB || deneb) seg(col, WH_EXEC, kWireExec[k].rec, o, kWireExec[k].len), o += kWireExec[k].len;
  }
  seg(col, WH_EXEC, K_EXEC_EXTRA_OFF, o, elen);
  return o + elen;
}
// The fixed part; att / fin: the values of the two headers' offset fields.  `image`: the offsets are those of the
// kernels' LDS image, which has the committee cut out (the committee is then no segment).  joined(a, alen, b): the
// caller keeps column b directly behind the alen bytes of column a; pieces that the same kinds carry one behind the
// other (bits, signature, slot) and that the caller keeps so are handed over as one segment, under the first column
constexpr bool wire_pair(uint32_t k) {  // pieces k - 1 and k: plain, and always together
  return k > 0 && k < WIRE_PIECES && kWirePieces[k].len && kWirePieces[k - 1].len && kWirePieces[k].kinds == kWirePieces[k - 1].kinds;
}
template <class Seg, class Put, class Joined>
LCV_WIRE_FN uint32_t wire_walk_fixed(uint32_t kind, bool altair, bool image, uint32_t att, uint32_t fin, Seg seg, Put put, Joined joined) {
  auto glued = [&](uint32_t k) { return wire_pair(k) && joined(kWirePieces[k - 1].col, kWirePieces[k - 1].len, kWirePieces[k].col); };
  uint32_t o = 0;
  LCV_WIRE_UNROLL for (uint32_t k = 0; k < WIRE_PIECES; ++k) {
    const uint32_t col = kWirePieces[k].col, len = wire_piece_len(k, altair);
    if (!((kWirePieces[k].kinds >> kind) & 1u) || (image && col == WC_COMMITTEE)) continue;
    if (!kWirePieces[k].len && !altair) {
      put(o, col == WC_ATT ? att : fin);
    } else if (!glued(k)) {  // (a glued piece went with the one before it)
      uint32_t n = len;
      LCV_WIRE_UNROLL for (uint32_t j = k + 1; j < WIRE_PIECES && glued(j); ++j) n += kWirePieces[j].len;
      seg(col, WH_BEACON, 0u, o, n);
    }
    o += len;
  }
  return o;
}

// ---- what is well-formed, as upstream SSZ deserialisation has it: the first offset equals the fixed size, offsets
// are monotonic and in bounds, no trailing bytes, the header's offset is its fixed size, extra_data's offset is the
// ExecutionPayloadHeader's fixed size, extra_data has at most 32 bytes.  The offsets inside a message are a peer's:
// they are compared as unsigned values against the length and added to nothing before that, and no read through
// rd(o) — the little-endian u32 at message offset o — comes before the length check that covers o + 4.
constexpr bool wire_len_ok(uint32_t kind, uint32_t fork, uint64_t len) {  // decided before any read
  return wire_fork_ok(fork) && (fork == WIRE_ALTAIR ? len == wire_msg_fixed(kind, true)
                                                    : len >= wire_msg_fixed(kind, false) && len <= wire_msg_max(kind, fork));
}
// status 0: the two headers as (offset in the message, length) and their extra_data lengths; status 1: malformed
struct WirePlan { uint32_t status, att_off, att_len, fin_off, fin_len, elen_att, elen_fin; };

template <class Rd>
LCV_WIRE_FN bool wire_header_ok(Rd rd, uint32_t h, uint32_t hlen, bool deneb, uint32_t* elen) {
  const uint32_t fixed = wire_header_fixed() + wire_exec_fixed(deneb);
  if (hlen < fixed || hlen - fixed > (uint32_t)K_MAX_EXTRA) return false;  // every read lies below h + fixed
  if (rd(h + wire_header_offset_pos()) != wire_header_fixed()) return false;
  if (rd(h + wire_header_fixed() + wire_exec_offset_pos()) != wire_exec_fixed(deneb)) return false;
  *elen = hlen - fixed;
  return true;
}
template <class Rd>
LCV_WIRE_FN WirePlan wire_accept(uint32_t kind, uint32_t fork, uint64_t len64, Rd rd) {
  WirePlan p = {1u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (!wire_len_ok(kind, fork, len64)) return p;
  if (fork == (uint32_t)WIRE_ALTAIR) {  // fixed-size: the length was the whole check
    p.status = 0u;
    return p;
  }
  const uint32_t len = (uint32_t)len64, fixed = wire_msg_fixed(kind, false);
  const bool fin = wire_has(WC_FIN, kind), deneb = fork == (uint32_t)WIRE_DENEB;
  const uint32_t a0 = rd(wire_piece_pos(WC_ATT, kind, false));
  if (a0 != fixed) return p;
  // the second offset is any 32-bit value (0x80000000, 0xFFFFFFFF): compared, never added to
  const uint32_t a1 = fin ? rd(wire_piece_pos(WC_FIN, kind, false)) : len;
  if (a1 < a0 || a1 > len) return p;
  p.att_off = a0, p.att_len = a1 - a0, p.fin_off = a1, p.fin_len = len - a1;
  if (!wire_header_ok(rd, p.att_off, p.att_len, deneb, &p.elen_att)) return p;
  if (fin && !wire_header_ok(rd, p.fin_off, p.fin_len, deneb, &p.elen_fin)) return p;
  p.status = 0u;
  return p;
}

}  // namespace lcv
