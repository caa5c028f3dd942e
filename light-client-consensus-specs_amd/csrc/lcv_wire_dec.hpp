// lcv_wire_dec.hpp — SSZ wire messages into the rows of a resident batch on the device (lcv_batch_decode,
// include/lcv.h): F_wire_enc (lcv_wire_enc.hpp) run backwards.  lcv_wire_layout.hpp describes the containers and what
// is malformed (wire_accept, which the host decoder lcv_wire.cpp runs too); the offsets inside a message are a
// peer's, so every one of them is checked against the message's length before anything is read through it.
//
// The driver stages message i at a 16-byte aligned offset of one device scratch and hands the kernels
// (dev_off[i], len[i], fork[i]) (DEC_META_BYTES per message).  Four functors, 64-lane teams:
//
// F_wire_dec, one team per message, over one LDS area (DEC_LDS_WORDS):
//   round 0  the row's raw area (the encoder's ENC_R_* layout) zeroed; a length the kind and fork cannot have is
//            decided from `len` alone, before any load; else the message WITHOUT its committee, global -> LDS
//            "image" in aligned 16-byte loads (K_SC is a multiple of 16, so a byte behind the committee keeps its
//            offset modulo 16).  No load starts at or past dev_off + round_up(len, 16)
//   round 1  every lane derives the same plan from the image (wire_accept, the host decoder's rule; offsets compared as
//            unsigned values against the length, never added to anything first); lane 0 keeps the status in DEC_CTL
//            and stores the row's 16-byte record; the team moves the pieces image -> raw inside LDS, 4 bytes at a
//            time, or 1 where an offset or a length is odd (the finalized header starts at any residue).  Only bytes
//            below `len` are moved, so what lies past a message in the scratch never reaches a row
//   round 2  DEC_ROWS: raw -> the byte columns in aligned 16-byte stores and signature_slot; a malformed row stores
//            zeros.  DEC_PLAN (updates only): the committee as 16-byte loads at message offset 4 (dword aligned) or 112
//            (Altair), each lane folding (word index, word) into a 64-bit hash and an OR, kept per lane in LDS
//   round 3  DEC_PLAN: lane 0 combines the lanes' values in lane order; the record gains `zero` and `hash`
// F_wire_relay, one team per (message, store) pair and one per message: F_wire_dec's rounds through a row map.
// F_sc_confirm, one team per listed pair: two committees of the scratch compared, one flag.
// F_sc_gather, one team per pool row: the representative's committee into the pool, aligned 16-byte stores; the
//   sentinel DEC_NO_COMMITTEE gives the all-zero row (SyncCommittee()).
// No round reads LDS that the same round writes.
#pragma once
#include "lcv_wire_enc.hpp"

namespace lcv {

enum : uint32_t {
  DEC_TEAM = 64,
  DEC_RAW_BYTES = ENC_R_SLOT + 16,
  DEC_LANES = DEC_RAW_BYTES,             // per lane 16 bytes: hash low, hash high, OR of the words, 0
  DEC_CTL = DEC_LANES + 16 * DEC_TEAM,   // status, the committee's offset in the message
  DEC_IMG = DEC_CTL + 16,
  DEC_IMG_BYTES = ENC_IMG_BYTES,
  DEC_LDS_WORDS = (DEC_IMG + DEC_IMG_BYTES) / 4,
  DEC_META_BYTES = 16,  // per message: u64 offset in the scratch, u32 length, u32 fork code
  DEC_REC_BYTES = 16,   // per row: u32 status, u32 zero (no committee, or an all-zero one), u64 committee hash
  DEC_PAIR_BYTES = 16,  // F_sc_confirm: two u64 scratch offsets of committees
  DEC_PLAN = 0, DEC_ROWS = 1,
};
constexpr uint64_t DEC_NO_COMMITTEE = ~0ull;
static_assert(DEC_RAW_BYTES % 16 == 0 && DEC_IMG % 16 == 0, "16-byte LDS words");
static_assert(ENC_R_FIN % 16 == 0 && ENC_H_EXEC % 16 == 0 && ENC_H_BRANCH % 16 == 0 && ENC_R_NSC_BRANCH % 16 == 0 &&
              ENC_R_FIN_BRANCH % 16 == 0 && ENC_R_BITS % 16 == 0 && ENC_R_SIG % 16 == 0, "raw pieces leave in 16-byte words");

LCV_FN uint32_t dec_rd32(const uint8_t* img, uint32_t o) {
  return (uint32_t)img[o] | ((uint32_t)img[o + 1] << 8) | ((uint32_t)img[o + 2] << 16) | ((uint32_t)img[o + 3] << 24);
}
LCV_FN uint64_t dec_mix(uint64_t h, uint64_t x) {
  h = (h ^ x) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

struct DecMeta { uint64_t off; uint32_t len, fork; };
LCV_FN DecMeta dec_meta(const uint8_t* meta, uint32_t i) {
  const q128 m = ld_q128(meta, i);
  DecMeta r;
  r.off = (uint64_t)m.x | ((uint64_t)m.y << 32);
  r.len = m.z;
  r.fork = m.w;
  return r;
}

// ---- round 1's moves inside LDS: img[src .. src + len) -> raw[dst ..), the team's lanes striding over dwords, or
// over bytes where src or len is no multiple of 4 (dst always is)
LCV_FN void dec_seg(uint8_t* raw, uint32_t dst, const uint8_t* img, uint32_t src, uint32_t len, uint32_t lane) {
  if (((src | len) & 3u) == 0u) {
    for (uint32_t k = lane; k < len / 4; k += DEC_TEAM) ((uint32_t*)(raw + dst))[k] = ((const uint32_t*)(img + src))[k];
  } else {
    for (uint32_t k = lane; k < len; k += DEC_TEAM) raw[dst + k] = img[src + k];
  }
}

// round 2's move: 16-byte words LDS -> global, zeros for a malformed row
LCV_FN void dec_store(uint8_t* dst, const uint8_t* raw, uint32_t bytes, uint32_t lane, bool ok) {
  for (uint32_t k = lane; k < bytes / 16; k += DEC_TEAM) {
    q128 v = {0u, 0u, 0u, 0u};
    if (ok) v = lds_q128(raw, k);
    st_q128(dst, k, v);
  }
}

struct DecArgs {
  const uint8_t* stage;  // the staged messages
  const uint8_t* meta;   // [n][DEC_META_BYTES]
  uint8_t* rec;          // [n][DEC_REC_BYTES], or null: not wanted
  ProdOut O;             // DEC_ROWS: the batch's row columns
  uint32_t kind, phase;
};

// (`kind` is A.kind as a constant of the call: one instance per kind, as F_wire_enc.)  The rounds, for message i into
// row `row` of the columns: F_wire_dec's team decodes message i into row i; F_wire_relay's takes its message from a row
// map (lcv_relay_async).  `recs`: the message's record, or null: not wanted
LCV_FN void item_wire_dec_to(uint32_t i, uint32_t row, uint8_t* recs, uint32_t lane, uint32_t r, uint32_t* lds, const DecArgs& A,
                             const uint32_t kind) {
  uint8_t* raw = (uint8_t*)lds;
  uint8_t* img = raw + DEC_IMG;
  const DecMeta M = dec_meta(A.meta, i);
  const bool upd = wire_has(WC_COMMITTEE, kind), altair = M.fork == (uint32_t)WIRE_ALTAIR;
  const uint32_t coff = wire_committee_off(altair);  // an update's committee, in the message
  const uint32_t cut = upd ? (uint32_t)K_SC : 0u;    // what the image leaves out
  if (r == 0) {
    const q128 z = {0u, 0u, 0u, 0u};
    for (uint32_t k = lane; k < DEC_RAW_BYTES / 16; k += DEC_TEAM) st_q128(raw, k, z);
    if (!wire_len_ok(kind, M.fork, M.len)) return;  // a length the kind and fork cannot have fits no image
    const uint8_t* src = A.stage + M.off;
    const uint32_t imglen = M.len - cut;
    // image word w: message word w before the committee, w + ENC_SC_WORDS behind it; word 0 of a Deneb / Capella
    // update is the first offset and then what follows the committee's last dword.  The highest message word read
    // is ceil(len / 16) - 1
    for (uint32_t w = lane; w < (imglen + 15u) / 16u; w += DEC_TEAM) {
      q128 v;
      if (!upd) {
        v = ld_q128(src, w);
      } else if (altair) {
        v = ld_q128(src, w < coff / 16u ? w : w + ENC_SC_WORDS);
      } else {
        v = ld_q128(src, w + ENC_SC_WORDS);
        if (w == 0u) v.x = ld_q128(src, 0).x;
      }
      st_q128(img, w, v);
    }
    return;
  }
  if (r == 1) {
    // the message is read through the image: an offset behind the committee lies K_SC lower there
    const WirePlan p = wire_accept(kind, M.fork, M.len, [&](uint32_t o) { return dec_rd32(img, o < coff ? o : o - cut); });
    if (lane == 0) {
      lds[DEC_CTL / 4] = p.status;
      if (recs) {
        const q128 v = {p.status, 1u, 0u, 0u};
        st_q128(recs, i, v);
      }
    }
    if (p.status) return;
    auto seg = [&](uint32_t col, uint32_t part, uint32_t rec, uint32_t at, uint32_t len) {
      dec_seg(raw, enc_raw_of(col, part) + rec, img, at, len, lane);
    };
    auto put = [](uint32_t, uint32_t) {};  // (the offsets were wire_accept's to check)
    if (altair) {  // every container fixed-size: fields in order
      wire_walk_fixed(kind, true, true, 0u, 0u, seg, put, EncRawJoined());
      return;
    }
    // the encoder's walk backwards: the header at img[at ..) into its raw header (the record's gaps stay zero)
    auto header = [&](uint32_t col, uint32_t at, uint32_t elen) {
      wire_walk_header(col, at, M.fork == (uint32_t)WIRE_DENEB, elen, seg, put);
      if (lane == 0) *(uint32_t*)(raw + enc_raw_of(col, WH_EXEC) + K_EXEC_EXTRALEN_OFF) = elen;
    };
    // (the attested header follows the fixed part, as wire_accept checked: a constant of the kind, not p.att_off - cut)
    header(WC_ATT, wire_walk_fixed(kind, false, true, 0u, 0u, seg, put, EncRawJoined()), p.elen_att);
    if (wire_has(WC_FIN, kind)) header(WC_FIN, p.fin_off - cut, p.elen_fin);
    return;
  }
  const bool ok = lds[DEC_CTL / 4] == 0u;
  if (A.phase == (uint32_t)DEC_ROWS) {  // round 2: the row
    const ProdOut& O = A.O;
    const size_t s = row;
    dec_store(O.att_beacon + (size_t)K_BEACON * s, raw + ENC_R_ATT + ENC_H_BEACON, K_BEACON, lane, ok);
    dec_store(O.att_exec + (size_t)K_EXEC * s, raw + ENC_R_ATT + ENC_H_EXEC, K_EXEC, lane, ok);
    dec_store(O.att_branch + (size_t)K_EXEC_BRANCH * s, raw + ENC_R_ATT + ENC_H_BRANCH, K_EXEC_BRANCH, lane, ok);
    dec_store(O.fin_beacon + (size_t)K_BEACON * s, raw + ENC_R_FIN + ENC_H_BEACON, K_BEACON, lane, ok);
    dec_store(O.fin_exec + (size_t)K_EXEC * s, raw + ENC_R_FIN + ENC_H_EXEC, K_EXEC, lane, ok);
    dec_store(O.fin_branch + (size_t)K_EXEC_BRANCH * s, raw + ENC_R_FIN + ENC_H_BRANCH, K_EXEC_BRANCH, lane, ok);
    dec_store(O.nsc_branch + (size_t)K_NSC_BRANCH * s, raw + ENC_R_NSC_BRANCH, K_NSC_BRANCH, lane, ok);
    dec_store(O.finality_branch + (size_t)K_FIN_BRANCH * s, raw + ENC_R_FIN_BRANCH, K_FIN_BRANCH, lane, ok);
    dec_store(O.bits + (size_t)K_BITS * s, raw + ENC_R_BITS, K_BITS, lane, ok);
    dec_store(O.sig + (size_t)K_SIG * s, raw + ENC_R_SIG, K_SIG, lane, ok);
    if (lane == 0)
      O.sig_slot[s] = ok ? (uint64_t)lds[ENC_R_SLOT / 4] | ((uint64_t)lds[ENC_R_SLOT / 4 + 1] << 32) : 0ull;
    return;
  }
  // DEC_PLAN (updates): the committee's hash.  A row that passed has len >= coff + K_SC
  if (!ok) return;
  if (r == 2) {
    const uint8_t* sc = A.stage + M.off + coff;
    uint64_t h = dec_mix(0x6c63765f77646563ull, lane);
    uint32_t any = 0;
    for (uint32_t w = lane; w < (uint32_t)ENC_SC_WORDS; w += DEC_TEAM) {
      const q128 v = ld_q128_dw(sc + 16 * (size_t)w);
      h = dec_mix(h, w);
      h = dec_mix(h, (uint64_t)v.x | ((uint64_t)v.y << 32));
      h = dec_mix(h, (uint64_t)v.z | ((uint64_t)v.w << 32));
      any |= v.x | v.y | v.z | v.w;
    }
    const q128 mine = {(uint32_t)h, (uint32_t)(h >> 32), any, 0u};
    st_q128(raw + DEC_LANES, lane, mine);
    return;
  }
  if (lane == 0) {  // round 3: the lanes' values in lane order
    uint64_t h = 0;
    uint32_t any = 0;
    LCV_NOUNROLL for (uint32_t l = 0; l < DEC_TEAM; ++l) {
      const q128 v = lds_q128(raw + DEC_LANES, l);
      h = dec_mix(h, (uint64_t)v.x | ((uint64_t)v.y << 32));
      any |= v.z;
    }
    const q128 v = {0u, any ? 0u : 1u, (uint32_t)h, (uint32_t)(h >> 32)};
    st_q128(recs, i, v);
  }
}
LCV_FN void item_wire_dec(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, const DecArgs& A, const uint32_t kind) {
  item_wire_dec_to(i, i, A.rec, lane, r, lds, A, kind);
}

// ---- the relay's decode with a row map (lcv_relay_async): team i < npairs decodes message rows[i] straight into row
// i of the slot's table batch — no batch of nmsg rows in between, no gather launch: a message relayed to many stores is
// read that often from L2 — and team npairs + j runs rounds 0 and 1 for message j alone and stores its record, so that
// every message has its status, named by a pair or not, and each record has one writer.  rows[i] < nmsg is the
// driver's check, before the launch
struct RelayDecArgs {
  DecArgs D;             // phase DEC_ROWS; rec: [nmsg]; O: the npairs rows' columns
  const uint32_t* rows;  // [npairs]
  uint32_t npairs;
};
LCV_FN void item_wire_relay(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, const RelayDecArgs& A, const uint32_t kind) {
  const bool pair = i < A.npairs;
  if (!pair && r >= 2u) return;  // a status team has no row
  item_wire_dec_to(pair ? A.rows[i] : i - A.npairs, i, pair ? nullptr : A.D.rec, lane, r, lds, A.D, kind);
}

// ---- the pool: full compares of candidate committees, and the gather of the distinct ones
struct ScConfirmArgs {
  const uint8_t* stage;
  const uint8_t* pairs;  // [m][DEC_PAIR_BYTES]: the scratch offsets (multiples of 4) of two committees
  uint32_t* differ;      // [m]: 1 where they differ
};
LCV_FN void item_sc_confirm(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, const ScConfirmArgs& A) {
  if (r == 0) {
    const q128 p = ld_q128(A.pairs, i);
    const uint8_t* a = A.stage + ((uint64_t)p.x | ((uint64_t)p.y << 32));
    const uint8_t* b = A.stage + ((uint64_t)p.z | ((uint64_t)p.w << 32));
    uint32_t d = 0;
    for (uint32_t w = lane; w < (uint32_t)ENC_SC_WORDS; w += DEC_TEAM) {
      const q128 x = ld_q128_dw(a + 16 * (size_t)w), y = ld_q128_dw(b + 16 * (size_t)w);
      d |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    lds[lane] = d;
    return;
  }
  if (lane == 0) {
    uint32_t d = 0;
    LCV_NOUNROLL for (uint32_t k = 0; k < DEC_TEAM / 4; ++k) {
      const q128 v = lds_q128((const uint8_t*)lds, k);
      d |= v.x | v.y | v.z | v.w;
    }
    A.differ[i] = d ? 1u : 0u;
  }
}

struct ScGatherArgs {
  const uint8_t* stage;
  const uint64_t* src;  // [npool]: the scratch offset of the pool row's committee, or DEC_NO_COMMITTEE
  uint8_t* pool;        // [npool][K_SC]
};
LCV_FN void item_sc_gather(uint32_t i, uint32_t lane, const ScGatherArgs& A) {
  const uint64_t s = A.src[i];
  uint8_t* dst = A.pool + (size_t)K_SC * i;
  for (uint32_t w = lane; w < (uint32_t)ENC_SC_WORDS; w += DEC_TEAM) {
    q128 v = {0u, 0u, 0u, 0u};
    if (s != DEC_NO_COMMITTEE) v = ld_q128_dw(A.stage + s + 16 * (size_t)w);
    st_q128(dst, w, v);
  }
}

}  // namespace lcv

// ---- the kernels' functors (LCV_HD: __device__ in lcv_k_dec.hip, empty in the host simulation)
struct F_wire_dec {
  lcv::DecArgs A;
  static constexpr uint32_t TEAM = lcv::DEC_TEAM, LDS_WORDS = lcv::DEC_LDS_WORDS, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return A.phase == (uint32_t)lcv::DEC_PLAN ? 4u : 3u; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, uint32_t*) const {
    if (A.kind == (uint32_t)lcv::WIRE_UPDATE) lcv::item_wire_dec(i, lane, r, lds, A, lcv::WIRE_UPDATE);
    else if (A.kind == (uint32_t)lcv::WIRE_FINALITY) lcv::item_wire_dec(i, lane, r, lds, A, lcv::WIRE_FINALITY);
    else lcv::item_wire_dec(i, lane, r, lds, A, lcv::WIRE_OPTIMISTIC);
  }
};
struct F_wire_relay {  // (the gossip kinds only: a full update's committee pool needs the host in between)
  lcv::RelayDecArgs A;
  static constexpr uint32_t TEAM = lcv::DEC_TEAM, LDS_WORDS = lcv::DEC_LDS_WORDS, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return 3u; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, uint32_t*) const {
    if (A.D.kind == (uint32_t)lcv::WIRE_FINALITY) lcv::item_wire_relay(i, lane, r, lds, A, lcv::WIRE_FINALITY);
    else lcv::item_wire_relay(i, lane, r, lds, A, lcv::WIRE_OPTIMISTIC);
  }
};
struct F_sc_confirm {
  lcv::ScConfirmArgs A;
  static constexpr uint32_t TEAM = lcv::DEC_TEAM, LDS_WORDS = lcv::DEC_TEAM, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return 2u; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, uint32_t*) const {
    lcv::item_sc_confirm(i, lane, r, lds, A);
  }
};
struct F_sc_gather {
  lcv::ScGatherArgs A;
  static constexpr uint32_t TEAM = lcv::DEC_TEAM, LDS_WORDS = 4, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return 1u; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t, uint32_t*, uint32_t*) const {
    lcv::item_sc_gather(i, lane, A);
  }
};
