// lcv_rlc.hpp — device side of randomised batch verification (lcv_set_rlc, include/lcv.h "Batch verification").
// For a group of G consecutive items of a chunk, with secret 64-bit coefficients r_i,
//     prod_i e(r_i PK_i, H(m_i)) e(r_i (-G1), S_i) == 1
// holds when every item of the group is valid and fails otherwise except with probability about 2^-64, so a group
// pays ONE final exponentiation; only the items of a failing group pay one of their own.  The scaling touches G1
// points only: the line walks, the accumulation and the final-exponentiation program run as they are, on Work views.
//   F_rlc_scale      one lane per item: r_i PK_i -> pk_s, r_i (-G1) -> g1_s (affine, one shared inversion)
//   F_sop_lines_g1   F_sop_lines' signature walk with the item's own second point (g1_s) instead of -G1
//   F_sop_f12mul     one level of the product tree over a group's Miller values (program f12mul)
//   F_rlc_spread     a passing group's items get pair_ok = 1, a failing group's items are listed in retry[]
//   F_sop_fexp_rows  the unchanged final exponentiation over the rows retry[] lists (k_sop_counted: their number
//                    stays on the device)
#pragma once
#include "lcv_functors_sop.hpp"

namespace lcv {

// the slot's scratch (lcv_driver.inc ensure_rlc, kRlcFields); cap is the slot's work-space capacity, so pk_s and
// g1_s are addressed like W.pk
struct RlcDev {
  uint32_t* pk_s;    // [24][cap] r_i PK_i affine
  uint32_t* g1_s;    // [24][cap] r_i (-G1) affine
  uint32_t* prod_a;  // [cap][144] the product tree's levels, ping
  uint32_t* prod_b;  // [cap][144] ... pong (a level written in place would race with its own reads)
  uint8_t* g_ok;     // [cap] the groups' "== 1"
  uint32_t* retry;   // [cap] the items of failing groups, in any order
  uint32_t* cnt;     // [4] 0: entries of retry[] (this chunk); 1: the same, summed over the batch's chunks
};

// what the coefficients of one chunk are derived from: lcv_set_rlc's seed (as big-endian words) and the context's
// batch counter of the chunk
struct RlcKey { uint32_t seed[8]; uint64_t counter; };

// r_i = the first 8 bytes, little-endian, of SHA-256(seed32 || counter (u64 LE) || i (u32 LE)), 0 replaced by 1:
// 44 bytes, one compression
LCV_FN uint64_t rlc_coeff(const RlcKey& K, uint32_t i) {
  uint32_t st[8], blk[16];
  sha256_iv(st);
  LCV_UNROLL for (int k = 0; k < 8; ++k) blk[k] = K.seed[k];
  blk[8] = bswap32((uint32_t)K.counter);
  blk[9] = bswap32((uint32_t)(K.counter >> 32));
  blk[10] = bswap32(i);
  blk[11] = 0x80000000u;
  blk[12] = blk[13] = blk[14] = 0;
  blk[15] = 44 * 8;
  sha256_compress(st, blk);
  const uint64_t r = (uint64_t)bswap32(st[0]) | ((uint64_t)bswap32(st[1]) << 32);
  return r ? r : 1ull;
}

// ra = r p, rb = r q for affine p, q of prime order and 0 < r < 2^64: two select-per-bit ladders (as
// jac_mul_scalar_be32) side by side, then both to affine with one inversion (Montgomery's trick).  A result at
// infinity (never, under those conditions) comes out as (0, 0)
LCV_FN void rlc_scale_pair(g1a& ra, g1a& rb, const g1a& p, const g1a& q, uint64_t r) {
  g1j a, b;
  jac_set_inf(a);
  jac_set_inf(b);
  LCV_NOUNROLL for (int bit = 63; bit >= 0; --bit) {
    const bool set = (r >> bit) & 1ull;
    g1j t;
    jac_dbl(a, a);
    jac_madd(t, a, p);
    if (set) a = t;
    jac_dbl(b, b);
    jac_madd(t, b, q);
    if (set) b = t;
  }
  fp zz, zi, za, zb, z2;
  fp_mul(zz, a.z, b.z);
  fp_inv(zi, zz);
  fp_mul(za, zi, b.z);  // 1 / a.z
  fp_mul(zb, zi, a.z);  // 1 / b.z
  fp_sqr(z2, za);
  fp_mul(ra.x, a.x, z2);
  fp_mul(z2, z2, za);
  fp_mul(ra.y, a.y, z2);
  fp_sqr(z2, zb);
  fp_mul(rb.x, b.x, z2);
  fp_mul(z2, z2, zb);
  fp_mul(rb.y, b.y, z2);
  if (fp_is_zero(zz)) {
    fp_zero(ra.x); fp_zero(ra.y); fp_zero(rb.x); fp_zero(rb.y);
  }
}

// item i's scaled points; an item without an aggregate key (it is excluded from its group) gets zeros
LCV_FN void item_rlc_scale(uint32_t i, const Work& W, const RlcKey& K, const RlcDev& R) {
  g1a pk, g, a, b;
  if (W.agg_status[i] != PT_OK) {
    fp_zero(a.x); fp_zero(a.y);
    b = a;
  } else {
    soa_ld_fp(pk.x, W.pk, W.cap, i, 0);
    soa_ld_fp(pk.y, W.pk, W.cap, i, 1);
    g1_neg_generator(g);
    rlc_scale_pair(a, b, pk, g, rlc_coeff(K, i));
  }
  soa_st_fp(R.pk_s, W.cap, i, 0, a.x);
  soa_st_fp(R.pk_s, W.cap, i, 1, a.y);
  soa_st_fp(R.g1_s, W.cap, i, 0, b.x);
  soa_st_fp(R.g1_s, W.cap, i, 1, b.y);
}

// An item is multiplied into its group exactly when its verdict reads pair_ok (item_verdict, item_verdict_dedup):
// it has an aggregate key, its signature decoded and lies in G2 (the signature walk's check ran before), and
// (RLC_PRE: pre-checks ran and the items are the rows) its pre-checks passed
enum : uint32_t { RLC_PRE = 1u };
LCV_FN bool rlc_included(const Work& W, uint32_t i, uint32_t flags) {
  if (W.agg_status[i] != PT_OK || W.sig_status[i] == PT_BAD) return false;
  return !(flags & RLC_PRE) || W.pre_reason[i] == 0;
}

LCV_FN uint32_t rlc_atomic_inc(uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicAdd(p, 1u);
#else
  return __atomic_fetch_add(p, 1u, __ATOMIC_RELAXED);
#endif
}

// item i of m after the groups' final exponentiation (g_ok[i >> shift]); the retried items' pair_ok is written by
// the retry launch
LCV_FN void item_rlc_spread(uint32_t i, const Work& W, const RlcDev& R, uint32_t shift, uint32_t flags) {
  const bool in = rlc_included(W, i, flags);
  const bool pass = in && R.g_ok[i >> shift] != 0;
  W.pair_ok[i] = pass ? 1 : 0;
  if (in && !pass) {
    R.retry[rlc_atomic_inc(R.cnt)] = i;
    rlc_atomic_inc(R.cnt + 1);
  }
}

}  // namespace lcv

struct F_rlc_scale {
  lcv::Work W; lcv::RlcKey K; lcv::RlcDev R;
  LCV_HD void operator()(uint32_t i) const { lcv::item_rlc_scale(i, W, K, R); }
};
struct F_rlc_spread {
  lcv::Work W; lcv::RlcDev R; uint32_t shift, flags;
  LCV_HD void operator()(uint32_t i) const { lcv::item_rlc_spread(i, W, R, shift, flags); }
};
// test hooks (lcv_debug_rlc_coeffs, lcv_debug_rlc_scale: r P through the scaling kernel's own ladder and inversion)
struct F_dbg_rlc_coeffs {
  lcv::RlcKey K; uint64_t* out;
  LCV_HD void operator()(uint32_t i) const { out[i] = lcv::rlc_coeff(K, i); }
};
struct F_dbg_rlc_scale {
  const uint8_t* p96; const uint64_t* r; uint8_t* out96;
  LCV_HD void operator()(uint32_t i) const {
    lcv::g1a p, g, a, b;
    lcv::fp_from_be48_mont(p.x, p96 + 96 * (size_t)i);
    lcv::fp_from_be48_mont(p.y, p96 + 96 * (size_t)i + 48);
    lcv::g1_neg_generator(g);
    lcv::rlc_scale_pair(a, b, p, g, r[i]);
    lcv::fp_to_be48(out96 + 96 * (size_t)i, a.x);
    lcv::fp_to_be48(out96 + 96 * (size_t)i + 48, a.y);
  }
};

// The signature pairing's walk e(r (-G1), S): F_sop_lines in mode 1 — the same program, the same epilogue with the
// G2 subgroup check — whose prologue then replaces the generator constants by (-x, y) of the item's point in g1_s,
// on the lanes that wrote them
struct F_sop_lines_g1 {
  Work W; SopView P; const uint32_t* g1_s;
  static constexpr uint32_t WAVES = F_sop_lines::WAVES;
  static constexpr uint32_t TEAM = F_sop_lines::TEAM, LDS_WORDS = F_sop_lines::LDS_WORDS,
                            SHARED_WORDS = F_sop_lines::SHARED_WORDS;
  LCV_HD F_sop_lines base() const { return F_sop_lines{W, P, 1u}; }
  LCV_HD const uint32_t* io_in(uint32_t t) const { return base().io_in(t); }
  LCV_HD uint32_t* io_out(uint32_t t) const { return base().io_out(t); }
  LCV_HD void prologue(uint32_t t, uint32_t lane, uint32_t* lds) const {
    base().prologue(t, lane, lds);
    if (W.sig_status[t] != PT_OK) return;  // an identity Q keeps P = (0, 0)
    for (uint32_t v = lane; v < 12; v += TEAM) {
      if (v < 10) continue;
      fp x;
      soa_ld_fp(x, g1_s, W.cap, t, v - 10);
      if (v == 10) fp_neg(x, x);
      const uint32_t slot = v == 10 ? LCV_SOP_LINES_SLOT_NXP : LCV_SOP_LINES_SLOT_YP;
      LCV_UNROLL for (int j = 0; j < 12; ++j) lds[12 * slot + j] = x.v[j];
    }
  }
  LCV_HD void epilogue(uint32_t t, uint32_t lane, const uint32_t* lds) const { base().epilogue(t, lane, lds); }
};

// One level of the product tree: item j <- values 2j and 2j + 1 of src (src_n values), into dst[j].  A value past the
// end is 1; at level 0 (src = W.f, the Miller values) so is the value of an item that is not multiplied in
// (rlc_included)
struct F_sop_f12mul {
  Work W; SopView P;
  const uint32_t* src; uint32_t* dst;
  uint32_t src_n, level, flags;
  static constexpr uint32_t WAVES = LCV_SOP_WAVES;
  static constexpr uint32_t TEAM = LCV_SOP_F12MUL_TEAM, LDS_WORDS = LCV_SOP_F12MUL_SLOTS * 12 + SOP_PITCH_PAD,
                            SHARED_WORDS = LCV_SOP_F12MUL_NCONST * 12;
  static_assert(LCV_SOP_F12MUL_SLOT_A0_0 == 0 && LCV_SOP_F12MUL_SLOT_A5_1 == 11, "a in slots 0..11");
  static_assert(LCV_SOP_F12MUL_SLOT_B0_0 == 12 && LCV_SOP_F12MUL_SLOT_B5_1 == 23, "b in slots 12..23");
  LCV_HD const uint32_t* io_in(uint32_t) const { return nullptr; }
  LCV_HD uint32_t* io_out(uint32_t) const { return nullptr; }
  LCV_HD void prologue(uint32_t j, uint32_t lane, uint32_t* lds) const {
    for (uint32_t s = lane; s < 24; s += TEAM) {
      const uint32_t idx = 2 * j + s / 12, c = s % 12;
      fp x;
      if (idx >= src_n || (level == 0 && !rlc_included(W, idx, flags))) {
        if (c == 0) fp_one(x);
        else fp_zero(x);
      } else {
        f12_ld_coeff(x.v, src, idx, c);
      }
      LCV_UNROLL for (int k = 0; k < 12; ++k) lds[12 * s + k] = x.v[k];
    }
  }
  LCV_HD void epilogue(uint32_t j, uint32_t lane, const uint32_t* lds) const {
    for (uint32_t s = lane; s < 12; s += TEAM) {
      uint32_t x[12];
      LCV_UNROLL for (int k = 0; k < 12; ++k) x[k] = lds[12 * s + k];
      f12_st_coeff(dst, j, s, x);
    }
  }
};

// F_sop_fexp over the rows rows[0 .. n): item t reads W.f[rows[t]] and writes W.pair_ok[rows[t]]
struct F_sop_fexp_rows {
  Work W; SopView P; const uint32_t* rows;
  static constexpr uint32_t WAVES = F_sop_fexp::WAVES;
  static constexpr uint32_t TEAM = F_sop_fexp::TEAM, LDS_WORDS = F_sop_fexp::LDS_WORDS,
                            SHARED_WORDS = F_sop_fexp::SHARED_WORDS;
  LCV_HD const uint32_t* io_in(uint32_t) const { return nullptr; }
  LCV_HD uint32_t* io_out(uint32_t) const { return nullptr; }
  LCV_HD void prologue(uint32_t t, uint32_t lane, uint32_t* lds) const { F_sop_fexp{W, P}.prologue(rows[t], lane, lds); }
  LCV_HD void epilogue(uint32_t t, uint32_t lane, const uint32_t* lds) const { F_sop_fexp{W, P}.epilogue(rows[t], lane, lds); }
};

#ifdef LCV_KERNEL_UNIT
// k_sop's round loop (lcv_functors_sop.hpp; copied, so that k_sop compiles as it did) with the item count read from
// device memory: the host launches the worst-case grid without waiting for the count, and a block whose first item
// is at or past it returns before any barrier
template <class F>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(F::WAVES))) void k_sop_counted(F f, const uint32_t* n_dev, uint32_t g) {
  constexpr uint32_t T = F::TEAM, G = 64 / F::TEAM;
  if (g == 0 || g > G) g = G;
  const uint32_t n = __builtin_amdgcn_readfirstlane(*n_dev);
  if (blockIdx.x * g >= n) return;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t team = threadIdx.x / T, lane = threadIdx.x % T;
  const uint32_t item = blockIdx.x * g + team;
  const bool active = team < g && item < n;
  uint32_t* qp = lds + F::SHARED_WORDS;
  uint32_t* my = qp + lcv::SOP_QP_WORDS + (team < g ? team : 0) * F::LDS_WORDS;
  for (uint32_t k = threadIdx.x; k < F::SHARED_WORDS; k += 64) lds[k] = f.P.consts[k];
  if (threadIdx.x < lcv::SOP_QP_N) lcv::sop_qp_entry(qp + 16 * threadIdx.x, threadIdx.x);
  if (active) f.prologue(item, lane, my);
  __syncthreads();
  const uint32_t* io_in = active ? f.io_in(item) : nullptr;
  uint32_t* io_out = active ? f.io_out(item) : nullptr;
  const uint32_t R = f.P.rounds, ns = f.P.nslots;
  uint32_t h0 = 0, h3 = 0;
  const uint32_t* wn = f.P.rec;
  lcv::SopPre pre{0, 0, 0, 0, 0};
  if (R) {
    h0 = __builtin_amdgcn_readfirstlane(f.P.hdr[0]);
    const uint32_t off = __builtin_amdgcn_readfirstlane(f.P.hdr[1]);
    const uint32_t words = __builtin_amdgcn_readfirstlane(f.P.hdr[2]);
    h3 = __builtin_amdgcn_readfirstlane(f.P.hdr[3]);
    wn = f.P.rec + off + lane * words;
    if (active) pre = lcv::sop_pre(h0, wn);
  }
  for (uint32_t r = 0; r < R; ++r) {
    const uint32_t ch0 = h0, ch3 = h3;
    const uint32_t* w = wn;
    const lcv::SopPre cur = pre;
    if (r + 1 < R) {
      h0 = __builtin_amdgcn_readfirstlane(f.P.hdr[4 * r + 4]);
      const uint32_t off = __builtin_amdgcn_readfirstlane(f.P.hdr[4 * r + 5]);
      const uint32_t words = __builtin_amdgcn_readfirstlane(f.P.hdr[4 * r + 6]);
      h3 = __builtin_amdgcn_readfirstlane(f.P.hdr[4 * r + 7]);
      wn = f.P.rec + off + lane * words;
      if (active) pre = lcv::sop_pre(h0, wn);
    }
    if (active) lcv::sop_exec(ch0, ch3, w, cur, my, my, lds, ns, io_in, io_out, qp);
    __syncthreads();
  }
  if (active) f.epilogue(item, lane, my);
}
#endif
