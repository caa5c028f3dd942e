// lcv_wire_enc.hpp — SSZ wire bytes of a resident batch's rows on the device (lcv_batch_encode, include/lcv.h):
// LightClientUpdate / FinalityUpdate / OptimisticUpdate of the Deneb, Capella or Altair namespace, the fork forced
// for the call or chosen per row from the attested slot.  lcv_wire_layout.hpp describes the containers; the bytes are
// checked against lcv/wire.py encode_updates and the reference-serialised messages, which share nothing with it.
//
// One 64-lane team per message, three rounds over one LDS area (ENC_LDS_WORDS):
//   round 0  the row's columns, everything but the committee, global -> LDS "raw" in 16-byte loads; every lane
//            notes whether an execution record or branch word it moved was non-zero (ENC_FLAGS, a word per lane)
//   round 1  every lane derives the same plan from the raw copy (fork, the two extra_data lengths, status,
//            length; lane 0 keeps it in ENC_CTL and stores the row's 16-byte result record), then the team lays
//            the message out in the LDS "image" WITHOUT the committee: K_SC is a multiple of 16, so a byte after
//            the committee keeps its offset modulo 16 when the committee is cut out.  Pieces land at any byte
//            offset (the finalized header follows extra_data), so these are LDS moves of 4 bytes, or 1 where an
//            offset or a length is odd.  The image's last word is zero-filled past the message's end.
//   round 2  the output area, word by word (16 bytes), every word of the pitch stored exactly once with one aligned
//            16-byte store: image words from LDS, committee words straight from the pool — unshifted under Altair
//            (the committee starts at byte 112), shifted by one dword otherwise (byte 4: destination word k is the
//            last dword of source word k - 1 and the first three of word k, read as ONE 16-byte load at source
//            offset 16 k - 4, which is dword aligned) — and zero words past the end.
// A refused row (status != 0) stores zero words only.  No round reads LDS that the same round writes.
#pragma once
#include "lcv_producer.hpp"  // q128, ld_q128, st_q128

namespace lcv {

enum {
  ENC_TEAM = 64, ENC_ROUNDS = 3,
  ENC_SC_WORDS = K_SC / 16,
  // the raw copy: a header is beacon, execution record, execution branch; bits, signature and slot are contiguous
  ENC_H_BEACON = 0, ENC_H_EXEC = K_BEACON, ENC_H_BRANCH = K_BEACON + K_EXEC, ENC_H_BYTES = K_BEACON + K_EXEC + K_EXEC_BRANCH,
  ENC_R_ATT = 0, ENC_R_FIN = ENC_H_BYTES, ENC_R_NSC_BRANCH = 2 * ENC_H_BYTES, ENC_R_FIN_BRANCH = ENC_R_NSC_BRANCH + K_NSC_BRANCH,
  ENC_R_BITS = ENC_R_FIN_BRANCH + K_FIN_BRANCH, ENC_R_SIG = ENC_R_BITS + K_BITS, ENC_R_SLOT = ENC_R_SIG + K_SIG,
  ENC_FLAGS = ENC_R_SLOT + 16, ENC_CTL = ENC_FLAGS + 4 * ENC_TEAM, ENC_IMG = ENC_CTL + 16,
  ENC_IMG_BYTES = wire_image_bytes(),  // the longest message without its committee, its last word zero-filled
  ENC_LDS_WORDS = (ENC_IMG + ENC_IMG_BYTES) / 4,
  ENC_META_BYTES = 16,  // per row: u32 length, u8 fork, u8 status, 2 zero bytes, 4 version bytes, 4 zero bytes
};
static_assert(ENC_IMG % 16 == 0 && ENC_FLAGS % 16 == 0 && K_SC % 16 == 0, "16-byte LDS words");
static_assert(wire_committee_off(true) % 16 == 0 && wire_committee_off(false) == 4, "round 2: the committee unshifted or one dword on");
// where part `part` of wire column `col` lies in the raw copy
constexpr uint32_t enc_raw_of(uint32_t col, uint32_t part) {
  return (col == WC_ATT ? ENC_R_ATT : col == WC_FIN ? ENC_R_FIN : col == WC_NSC_BRANCH ? ENC_R_NSC_BRANCH : col == WC_FIN_BRANCH ? ENC_R_FIN_BRANCH
          : col == WC_BITS ? ENC_R_BITS : col == WC_SIG ? ENC_R_SIG : ENC_R_SLOT) +
         (part == WH_EXEC ? ENC_H_EXEC : part == WH_BRANCH ? ENC_H_BRANCH : ENC_H_BEACON);
}
// wire_walk_fixed's `joined`: column b lies directly behind the alen bytes of column a (bits, signature and slot do)
struct EncRawJoined {
  constexpr bool operator()(uint32_t a, uint32_t alen, uint32_t b) const {
    return a != WC_COMMITTEE && enc_raw_of(a, WH_BEACON) + alen == enc_raw_of(b, WH_BEACON);
  }
};

// a 16-byte word of the team's LDS area (the address space named, so that no select between an LDS and a global
// source turns the access into a flat one)
LCV_FN q128 lds_q128(const uint8_t* p, uint32_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 t = ((const __attribute__((address_space(3))) uint4*)p)[k];
  q128 r;
  r.x = t.x; r.y = t.y; r.z = t.z; r.w = t.w;
  return r;
#else
  return ld_q128(p, k);
#endif
}

// 16 bytes of global memory at an address that is a multiple of 4 only: still one 16-byte load (global accesses
// of any width need dword alignment, no more)
LCV_FN q128 ld_q128_dw(const uint8_t* p) {
  q128 r;
#if defined(__HIP_DEVICE_COMPILE__)
  struct __attribute__((aligned(4))) dw4 { uint32_t x, y, z, w; };
  const dw4 t = *(const dw4*)p;
  r.x = t.x; r.y = t.y; r.z = t.z; r.w = t.w;
#else
  memcpy(&r, p, 16);
#endif
  return r;
}

struct EncPlan { uint32_t fork, status, hatt, hfin, elen_att, elen_fin, imglen, version; };

// the message's layout from the raw copy; the same value on every lane
LCV_FN EncPlan enc_plan(const uint32_t* lds, const NetConfig& cfg, uint32_t kind, int32_t fork_arg) {
  EncPlan p;
  const uint64_t epoch = epoch_of_slot((uint64_t)lds[ENC_R_ATT / 4] | ((uint64_t)lds[ENC_R_ATT / 4 + 1] << 32), cfg);
  p.version = fork_version_word(epoch, cfg);
  p.fork = fork_arg >= 0 ? (uint32_t)fork_arg
                         : epoch >= cfg.fork_epoch[FORK_DENEB] ? (uint32_t)WIRE_DENEB
                                                               : epoch >= cfg.fork_epoch[FORK_CAPELLA] ? (uint32_t)WIRE_CAPELLA : (uint32_t)WIRE_ALTAIR;
  const bool fin = wire_has(WC_FIN, kind);  // the finalized header is encoded
  const uint32_t cut = wire_has(WC_COMMITTEE, kind) ? (uint32_t)K_SC : 0u;
  uint32_t flags = 0;
  LCV_NOUNROLL for (uint32_t k = 0; k < (uint32_t)ENC_TEAM / 4; ++k) {
    const q128 v = lds_q128((const uint8_t*)lds + ENC_FLAGS, k);
    flags |= v.x | v.y | v.z | v.w;
  }
  p.elen_att = p.elen_fin = 0;
  p.status = 0;
  if (p.fork == (uint32_t)WIRE_ALTAIR) {  // LightClientHeader = {beacon}: an encoded header carries no execution data
    if ((flags & 1u) || (fin && (flags & 2u))) p.status = 1;
    p.hatt = p.hfin = K_BEACON;
    p.imglen = wire_msg_fixed(kind, true) - cut;
  } else {
    const uint32_t fixed = wire_header_fixed() + wire_exec_fixed(p.fork == (uint32_t)WIRE_DENEB);
    p.elen_att = lds[(ENC_R_ATT + ENC_H_EXEC + K_EXEC_EXTRALEN_OFF) / 4];
    if (fin) p.elen_fin = lds[(ENC_R_FIN + ENC_H_EXEC + K_EXEC_EXTRALEN_OFF) / 4];
    if (p.elen_att > (uint32_t)K_MAX_EXTRA || p.elen_fin > (uint32_t)K_MAX_EXTRA) p.status = 2;
    p.hatt = fixed + p.elen_att;
    p.hfin = fixed + p.elen_fin;
    p.imglen = wire_msg_fixed(kind, false) - cut + p.hatt + (fin ? p.hfin : 0u);
  }
  return p;
}

// ---- round 1's moves inside LDS: raw[src .. src + len) -> img[dst ..), the team's lanes striding over dwords, or
// over bytes where dst or len is no multiple of 4 (src always is)
LCV_FN void enc_seg(uint8_t* img, uint32_t dst, const uint8_t* raw, uint32_t src, uint32_t len, uint32_t lane) {
  if (((dst | len) & 3u) == 0u) {
    for (uint32_t k = lane; k < len / 4; k += ENC_TEAM) ((uint32_t*)(img + dst))[k] = ((const uint32_t*)(raw + src))[k];
  } else {
    for (uint32_t k = lane; k < len; k += ENC_TEAM) img[dst + k] = raw[src + k];
  }
}
LCV_FN void enc_put32(uint8_t* img, uint32_t dst, uint32_t v, uint32_t lane) {
  if (lane != 0) return;
  if ((dst & 3u) == 0u) {
    *(uint32_t*)(img + dst) = v;
  } else {
    LCV_UNROLL for (int k = 0; k < 4; ++k) img[dst + k] = (uint8_t)(v >> (8 * k));
  }
}

// round 0's move: 16-byte words global -> LDS; returns the OR of the words this lane moved
template <uint32_t TEAM>
LCV_FN uint32_t enc_load(uint8_t* raw, const uint8_t* src, uint32_t bytes, uint32_t lane) {
  uint32_t nz = 0;
  for (uint32_t k = lane; k < bytes / 16; k += TEAM) {
    const q128 v = ld_q128(src, k);
    st_q128(raw, k, v);
    nz |= v.x | v.y | v.z | v.w;
  }
  return nz;
}

struct EncArgs {
  BatchDev B;
  const uint32_t* rows;  // the chunk's row list, or null: rows base, base + 1, ...
  uint32_t base;
  uint8_t* out;          // [chunk rows][pitch]
  uint8_t* meta;         // [chunk rows][ENC_META_BYTES]
  NetConfig cfg;
  uint32_t kind;
  int32_t fork;          // WIRE_DENEB .. WIRE_ALTAIR, or -1: per row
  uint32_t pitch;
};

LCV_FN void item_wire_enc(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, const EncArgs& A) {
  uint8_t* raw = (uint8_t*)lds;
  uint8_t* img = raw + ENC_IMG;
  const BatchDev& B = A.B;
  const uint32_t kind = A.kind;
  const size_t s = A.rows ? (size_t)A.rows[i] : (size_t)A.base + i;
  if (r == 0) {
    uint32_t f = 0;
    enc_load<ENC_TEAM>(raw + ENC_R_ATT + ENC_H_BEACON, B.att_beacon + (size_t)K_BEACON * s, K_BEACON, lane);
    if (enc_load<ENC_TEAM>(raw + ENC_R_ATT + ENC_H_EXEC, B.att_exec + (size_t)K_EXEC * s, K_EXEC, lane) |
        enc_load<ENC_TEAM>(raw + ENC_R_ATT + ENC_H_BRANCH, B.att_branch + (size_t)K_EXEC_BRANCH * s, K_EXEC_BRANCH, lane))
      f |= 1u;
    if (wire_has(WC_FIN, kind)) {
      enc_load<ENC_TEAM>(raw + ENC_R_FIN + ENC_H_BEACON, B.fin_beacon + (size_t)K_BEACON * s, K_BEACON, lane);
      if (enc_load<ENC_TEAM>(raw + ENC_R_FIN + ENC_H_EXEC, B.fin_exec + (size_t)K_EXEC * s, K_EXEC, lane) |
          enc_load<ENC_TEAM>(raw + ENC_R_FIN + ENC_H_BRANCH, B.fin_branch + (size_t)K_EXEC_BRANCH * s, K_EXEC_BRANCH, lane))
        f |= 2u;
      enc_load<ENC_TEAM>(raw + ENC_R_FIN_BRANCH, B.finality_branch + (size_t)K_FIN_BRANCH * s, K_FIN_BRANCH, lane);
    }
    if (wire_has(WC_COMMITTEE, kind))
      enc_load<ENC_TEAM>(raw + ENC_R_NSC_BRANCH, B.nsc_branch + (size_t)K_NSC_BRANCH * s, K_NSC_BRANCH, lane);
    enc_load<ENC_TEAM>(raw + ENC_R_BITS, B.bits + (size_t)K_BITS * s, K_BITS, lane);
    enc_load<ENC_TEAM>(raw + ENC_R_SIG, B.sig + (size_t)K_SIG * s, K_SIG, lane);
    if (lane == 0) {
      const uint64_t slot = B.sig_slot[s];
      lds[ENC_R_SLOT / 4] = (uint32_t)slot;
      lds[ENC_R_SLOT / 4 + 1] = (uint32_t)(slot >> 32);
    }
    lds[ENC_FLAGS / 4 + lane] = f;
    return;
  }
  if (r == 1) {
    const EncPlan p = enc_plan(lds, A.cfg, kind, A.fork);
    if (lane == 0) {
      const uint32_t len = p.status ? 0u : p.imglen + (wire_has(WC_COMMITTEE, kind) ? (uint32_t)K_SC : 0u);
      lds[ENC_CTL / 4] = p.status;
      lds[ENC_CTL / 4 + 1] = p.fork;
      lds[ENC_CTL / 4 + 2] = p.imglen;
      const q128 m = {len, p.fork | (p.status << 8), bswap32(p.version), 0u};
      st_q128(A.meta, i, m);
    }
    if (p.status) return;
    auto seg = [&](uint32_t col, uint32_t part, uint32_t rec, uint32_t at, uint32_t len) {
      enc_seg(img, at, raw, enc_raw_of(col, part) + rec, len, lane);
    };
    auto put = [&](uint32_t at, uint32_t v) { enc_put32(img, at, v, lane); };
    // (one instance per kind: the offsets of the fixed part and of the attested header are then constants, and a
    // move's choice between dwords and bytes is made when the kernel is compiled)
    auto lay = [&](uint32_t k) -> uint32_t {
      if (p.fork == (uint32_t)WIRE_ALTAIR) return wire_walk_fixed(k, true, true, 0u, 0u, seg, put, EncRawJoined());  // no offsets
      const bool deneb = p.fork == (uint32_t)WIRE_DENEB;
      const uint32_t fixed = wire_msg_fixed(k, false);  // (the offsets count the committee)
      uint32_t at = wire_walk_fixed(k, false, true, fixed, fixed + p.hatt, seg, put, EncRawJoined());
      at = wire_walk_header(WC_ATT, at, deneb, p.elen_att, seg, put);
      if (wire_has(WC_FIN, k)) at = wire_walk_header(WC_FIN, at, deneb, p.elen_fin, seg, put);
      return at;
    };
    const uint32_t o = kind == (uint32_t)WIRE_UPDATE ? lay(WIRE_UPDATE) : kind == (uint32_t)WIRE_FINALITY ? lay(WIRE_FINALITY) : lay(WIRE_OPTIMISTIC);
    // o == p.imglen: zero to the end of the image's last word
    for (uint32_t k = o + lane; k < ((o + 15u) & ~15u); k += ENC_TEAM) img[k] = 0;
    return;
  }
  // round 2: the output area, every 16-byte word of the pitch once
  const bool ok = lds[ENC_CTL / 4] == 0u;
  const uint32_t fork = lds[ENC_CTL / 4 + 1], imglen = lds[ENC_CTL / 4 + 2];
  uint8_t* dst = A.out + (size_t)A.pitch * i;
  const uint32_t words = A.pitch / 16;
  if (!wire_has(WC_COMMITTEE, kind)) {
    for (uint32_t w = lane; w < words; w += ENC_TEAM) {
      q128 v = {0u, 0u, 0u, 0u};
      if (ok && 16u * w < imglen) v = lds_q128(img, w);
      st_q128(dst, w, v);
    }
    return;
  }
  const uint8_t* sc = B.nsc_pool + (size_t)K_SC * B.nsc_index[s];
  if (fork == (uint32_t)WIRE_ALTAIR) {  // the attested header's words, then the committee: unshifted
    const uint32_t cw = wire_committee_off(true) / 16u;
    for (uint32_t w = lane; w < words; w += ENC_TEAM) {
      q128 v = {0u, 0u, 0u, 0u};
      if (ok) {
        if (w < cw) v = lds_q128(img, w);
        else if (w < cw + ENC_SC_WORDS) v = ld_q128(sc, w - cw);
        else if (16u * (w - ENC_SC_WORDS) < imglen) v = lds_q128(img, w - ENC_SC_WORDS);
      }
      st_q128(dst, w, v);
    }
    return;
  }
  // the committee at byte 4: word w = the last dword of committee word w - 1 (the first offset for w = 0), then the
  // first three of committee word w (image bytes 4 .. 15 for w = ENC_SC_WORDS)
  for (uint32_t w = lane; w < words; w += ENC_TEAM) {
    q128 v = {0u, 0u, 0u, 0u};
    if (ok) {
      if (w == 0u) {
        const q128 b = ld_q128(sc, 0);
        v.x = lds[ENC_IMG / 4];
        v.y = b.x; v.z = b.y; v.w = b.z;
      } else if (w < (uint32_t)ENC_SC_WORDS) {
        v = ld_q128_dw(sc + 16 * (size_t)w - 4);
      } else if (w == (uint32_t)ENC_SC_WORDS) {
        v = lds_q128(img, 0);
        v.x = ld_q128(sc, ENC_SC_WORDS - 1u).w;
      } else if (16u * (w - ENC_SC_WORDS) < imglen) {
        v = lds_q128(img, w - ENC_SC_WORDS);
      }
    }
    st_q128(dst, w, v);
  }
}

}  // namespace lcv

// ---- the kernel's functor (LCV_HD: __device__ in lcv_k_enc.hip, empty in the host simulation)
struct F_wire_enc {
  lcv::EncArgs A;
  static constexpr uint32_t TEAM = lcv::ENC_TEAM, LDS_WORDS = lcv::ENC_LDS_WORDS, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return lcv::ENC_ROUNDS; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, uint32_t*) const {
    lcv::item_wire_enc(i, lane, r, lds, A);
  }
};
