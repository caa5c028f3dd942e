// lcv_fold.hpp — process_light_client_update after validation (sync-protocol.md:514-553) over a batch: a rank
// record per update (item_rank, one lane per update) and the fold of records and verdicts into the next store
// state — for one store (item_fold_team, one 64-lane team for the whole batch) or store by store over a
// store-table batch (item_fold_seg_team, one team per store present).  Semantics: include/lcv.h.
//   is_better_update (:260-311) is a lexicographic order on (key0, -attested_slot, -signature_slot), so "the first
//   best update" is the first arg-max of the rank, and the per-row loop becomes a scan up to the first row that
//   applies (:545-553).
#pragma once
#include "lcv_items.hpp"

namespace lcv {

enum : uint32_t {
  RANK_BYTES = 32,
  RANK_SUPER = 1u << 23,   // 3 n >= 2 * 512
  RANK_N_HI_SHIFT = 13,    // bits 22-13: n when not super
  RANK_REL_SC = 1u << 12,  // is_sync_committee_update && period(attested) == period(signature)
  RANK_FIN = 1u << 11,     // is_finality_update
  RANK_FIN_SC = 1u << 10,  // is_finality_update && period(finalized) == period(attested)
  RANK_N_MASK = 0x3ffu,    // bits 9-0: n
  RANK_F_SC = 1u,          // flags bit 0: is_sync_committee_update
};
struct RankRec { uint32_t key0, flags; uint64_t att, sig, fin; };
static_assert(sizeof(RankRec) == RANK_BYTES, "a rank record is 32 bytes");

// the fold's state and result, byte for byte lcv_fold_state / lcv_fold_result of include/lcv.h
struct FoldState {
  uint64_t optimistic_slot, previous_max, current_max;
  uint32_t has_best, best_key0;
  uint64_t best_att, best_sig;
};
struct FoldResult {
  FoldState next;
  uint64_t rows_consumed;
  int64_t apply_row, best_row, optimistic_row;
  uint64_t accepted_count;
};
enum : uint32_t { FOLD_RESULT_BYTES = 128 };  // W.fold_out (the result's 88 bytes, padded)
static_assert(sizeof(FoldState) == 48 && sizeof(FoldResult) == 88, "fold state 48 bytes, result 88");

// byte offset of item i's record in W.rank (item-major; the layout check addresses it through this)
LCV_HDFN size_t rank_index(size_t i) { return i * RANK_BYTES; }

LCV_FN void rank_st(uint8_t* base, size_t i, const RankRec& r) {
  uint8_t* d = base + rank_index(i);
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* q = (uint4*)d;  // two 16-byte stores
  q[0] = make_uint4(r.key0, r.flags, (uint32_t)r.att, (uint32_t)(r.att >> 32));
  q[1] = make_uint4((uint32_t)r.sig, (uint32_t)(r.sig >> 32), (uint32_t)r.fin, (uint32_t)(r.fin >> 32));
#else
  uint32_t* w = (uint32_t*)d;
  w[0] = r.key0; w[1] = r.flags;
  w[2] = (uint32_t)r.att; w[3] = (uint32_t)(r.att >> 32);
  w[4] = (uint32_t)r.sig; w[5] = (uint32_t)(r.sig >> 32);
  w[6] = (uint32_t)r.fin; w[7] = (uint32_t)(r.fin >> 32);
#endif
}
LCV_FN void rank_ld(RankRec& r, const uint8_t* base, size_t i) {
  const uint8_t* s = base + rank_index(i);
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = (const uint4*)s;
  const uint4 a = q[0], b = q[1];
  r.key0 = a.x; r.flags = a.y;
  r.att = (uint64_t)a.z | ((uint64_t)a.w << 32);
  r.sig = (uint64_t)b.x | ((uint64_t)b.y << 32);
  r.fin = (uint64_t)b.z | ((uint64_t)b.w << 32);
#else
  const uint32_t* w = (const uint32_t*)s;
  r.key0 = w[0]; r.flags = w[1];
  r.att = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
  r.sig = (uint64_t)w[4] | ((uint64_t)w[5] << 32);
  r.fin = (uint64_t)w[6] | ((uint64_t)w[7] << 32);
#endif
}

// is_better_update(a, b), level by level (:260-311): equal ranks are not better
LCV_FN bool rank_better(uint32_t ka, uint64_t atta, uint64_t siga, uint32_t kb, uint64_t attb, uint64_t sigb) {
  if (ka != kb) return ka > kb;
  if (atta != attb) return atta < attb;
  return siga < sigb;
}

// the rank record of update i: six columns of the batch (participation bits, the two branches' emptiness, the
// attested and finalized beacon slots, signature_slot) and the configuration's period length
LCV_FN void item_rank(uint32_t i, const BatchDev& B, const Params& P, const Work& W) {
  const uint32_t n = popcount_bits(B.bits + 64 * (size_t)i);
  const bool is_sc = !bytes_all_zero(B.nsc_branch + (size_t)K_NSC_BRANCH * i, K_NSC_BRANCH / 4);
  const bool is_fin = !bytes_all_zero(B.finality_branch + (size_t)K_FIN_BRANCH * i, K_FIN_BRANCH / 4);
  RankRec r;
  r.att = ld_le64(B.att_beacon + (size_t)K_BEACON * i);
  r.fin = ld_le64(B.fin_beacon + (size_t)K_BEACON * i);
  r.sig = B.sig_slot[i];
  const uint64_t att_period = period_of_slot(r.att, P.cfg);
  const bool super = 3u * n >= 2u * 512u;
  r.key0 = (super ? (uint32_t)RANK_SUPER : n << RANK_N_HI_SHIFT) |
           ((is_sc && att_period == period_of_slot(r.sig, P.cfg)) ? (uint32_t)RANK_REL_SC : 0u) |
           (is_fin ? (uint32_t)RANK_FIN : 0u) |
           ((is_fin && period_of_slot(r.fin, P.cfg) == att_period) ? (uint32_t)RANK_FIN_SC : 0u) | n;
  r.flags = is_sc ? (uint32_t)RANK_F_SC : 0u;
  rank_st(W.rank, i, r);
}

// The fold: one team of 64 lanes for the rows of one store (the whole batch, or a segment of a store-table batch),
// lane l owning the contiguous stripe of ceil(n / 64) positions [l L, (l + 1) L).  A lane never reads, in a round,
// an LDS word another lane writes in that round.
//   round 0  every lane: the first row of its stripe that applies, and the max participation over the stripe's
//            valid rows up to that row
//   round 1  lane 0: the 64 summaries in lane order -> t, the running max each lane starts from, lanes past t dead
//   round 2  live lanes: their stripe again, up to t, with that running max -> the stripe's first best row, its
//            optimistic candidate, its number of valid rows
//   round 3  lane 0: the candidates in lane order with strict comparisons (earlier rows win ties, the state's own
//            best wins ties) -> the result
enum : uint32_t {
  FOLD_TEAM = 64, FOLD_ROUNDS = 4, FOLD_NONE = 0xFFFFFFFFu,
  FOLD_O_FIRST = 0, FOLD_O_MAX = 64, FOLD_O_PREFIX = 128, FOLD_O_T = 192, FOLD_O_RUN = 193,
  FOLD_O_BEST = 256, FOLD_O_OPT = 320, FOLD_O_CNT = 384, FOLD_LDS = 448,
};
// The rows a fold walks, as a compile-time map from position j of the walk to a row of W.rank / W.verdict: every
// row of the batch in order (F_fold), or one store's rows of a store-table batch (F_fold_seg: a segment, the batch
// rows seg_row[0 .. len) in ascending order).  Positions are what the rounds compare and keep in LDS; round 3
// turns the positions it reports into batch rows.
struct FoldRowsAll { LCV_HD uint32_t operator()(uint32_t j) const { return j; } };
struct FoldRowsSeg { const uint32_t* row; LCV_HD uint32_t operator()(uint32_t j) const { return row[j]; } };
// rows [i0, i0 + FOLD_BLK) of a stripe ending at `end` (i0 < end): records and verdicts loaded together, before any
// is looked at, so a lane has FOLD_BLK rows' loads in flight (a lane's rows are 32 bytes apart, the lanes' a stripe
// apart: the loads do not coalesce, their latency is what the walk costs).  Rows past `end` read row end - 1 and
// count as invalid.
enum : uint32_t { FOLD_BLK = 8 };
template <class Rows>
LCV_FN void fold_ld_block(RankRec x[FOLD_BLK], uint8_t ok[FOLD_BLK], const Work& W, const Rows& rows, uint32_t i0,
                          uint32_t end) {
  LCV_UNROLL for (uint32_t k = 0; k < FOLD_BLK; ++k) {
    const bool in = i0 + k < end;
    const uint32_t i = rows(in ? i0 + k : end - 1);
    ok[k] = in ? W.verdict[i] : (uint8_t)0;
    rank_ld(x[k], W.rank, i);
  }
}
// n rows (positions 0 .. n - 1 of `rows`), the result to `out` (FOLD_RESULT_BYTES, 16-byte aligned)
template <class Rows>
LCV_FN void item_fold_rows(uint32_t lane, uint32_t r, uint32_t* lds, const Work& W, const Rows& rows, const FoldState& in,
                           uint64_t store_fin_slot, uint32_t next_known, uint32_t n, uint8_t* out) {
  const uint32_t L = (n + FOLD_TEAM - 1) / FOLD_TEAM;
  const uint32_t lo = lane * L < n ? lane * L : n;
  const uint32_t hi = n - lo < L ? n : lo + L;
  if (r == 0) {
    uint32_t first = FOLD_NONE, m = 0;
    LCV_NOUNROLL for (uint32_t i0 = lo; i0 < hi && first == FOLD_NONE; i0 += FOLD_BLK) {
      RankRec x[FOLD_BLK];
      uint8_t ok[FOLD_BLK];
      fold_ld_block(x, ok, W, rows, i0, hi);
      LCV_UNROLL for (uint32_t k = 0; k < FOLD_BLK; ++k) {
        if (first != FOLD_NONE || !ok[k]) continue;
        const uint32_t ni = x[k].key0 & RANK_N_MASK;
        if (ni > m) m = ni;
        const bool fin_next = !next_known && (x[k].flags & RANK_F_SC) && (x[k].key0 & RANK_FIN) && (x[k].key0 & RANK_FIN_SC);
        if ((x[k].key0 & RANK_SUPER) && (x[k].fin > store_fin_slot || fin_next)) first = i0 + k;
      }
    }
    lds[FOLD_O_FIRST + lane] = first;
    lds[FOLD_O_MAX + lane] = m;
  } else if (r == 1) {
    if (lane != 0) return;
    uint32_t run = (uint32_t)in.current_max, t = FOLD_NONE;
    for (uint32_t l = 0; l < FOLD_TEAM; ++l) {
      if (t != FOLD_NONE) {
        lds[FOLD_O_PREFIX + l] = FOLD_NONE;  // past the applying row: not consumed
        continue;
      }
      lds[FOLD_O_PREFIX + l] = run;
      const uint32_t m = lds[FOLD_O_MAX + l];
      if (m > run) run = m;
      t = lds[FOLD_O_FIRST + l];
    }
    lds[FOLD_O_T] = t;
    lds[FOLD_O_RUN] = run;
  } else if (r == 2) {
    uint32_t best = FOLD_NONE, opt = FOLD_NONE, cnt = 0;
    uint32_t run = lds[FOLD_O_PREFIX + lane];
    if (run != FOLD_NONE) {
      const uint32_t t = lds[FOLD_O_T];
      const uint32_t end = (t != FOLD_NONE && t + 1 < hi) ? t + 1 : hi;
      const uint32_t prev = (uint32_t)in.previous_max;
      uint64_t opt_att = in.optimistic_slot, b_att = 0, b_sig = 0;
      uint32_t b_key = 0;
      LCV_NOUNROLL for (uint32_t i0 = lo; i0 < end; i0 += FOLD_BLK) {
        RankRec x[FOLD_BLK];
        uint8_t ok[FOLD_BLK];
        fold_ld_block(x, ok, W, rows, i0, end);
        LCV_UNROLL for (uint32_t k = 0; k < FOLD_BLK; ++k) {
          if (!ok[k]) continue;
          const uint32_t ni = x[k].key0 & RANK_N_MASK;
          ++cnt;
          if (ni > run) run = ni;
          if (ni > ((prev > run ? prev : run) >> 1) && x[k].att > opt_att) {  // get_safety_threshold (:323-327)
            opt_att = x[k].att;
            opt = i0 + k;
          }
          if (best == FOLD_NONE || rank_better(x[k].key0, x[k].att, x[k].sig, b_key, b_att, b_sig)) {
            best = i0 + k;
            b_key = x[k].key0; b_att = x[k].att; b_sig = x[k].sig;
          }
        }
      }
    }
    lds[FOLD_O_BEST + lane] = best;
    lds[FOLD_O_OPT + lane] = opt;
    lds[FOLD_O_CNT + lane] = cnt;
  } else {
    if (lane != 0) return;
    const uint32_t t = lds[FOLD_O_T];
    FoldResult res;
    res.next = in;
    res.next.current_max = lds[FOLD_O_RUN];
    res.best_row = -1;
    res.optimistic_row = -1;
    res.accepted_count = 0;
    bool has = in.has_best != 0;
    uint32_t b_key = in.best_key0;
    uint64_t b_att = in.best_att, b_sig = in.best_sig, opt_att = in.optimistic_slot;
    for (uint32_t l = 0; l < FOLD_TEAM; ++l) {
      res.accepted_count += lds[FOLD_O_CNT + l];
      const uint32_t o = lds[FOLD_O_OPT + l], b = lds[FOLD_O_BEST + l];
      RankRec x;
      if (o != FOLD_NONE) {
        const uint32_t row = rows(o);
        rank_ld(x, W.rank, row);
        if (x.att > opt_att) {
          opt_att = x.att;
          res.optimistic_row = (int64_t)row;
        }
      }
      if (b != FOLD_NONE) {
        const uint32_t row = rows(b);
        rank_ld(x, W.rank, row);
        if (!has || rank_better(x.key0, x.att, x.sig, b_key, b_att, b_sig)) {
          has = true;
          b_key = x.key0; b_att = x.att; b_sig = x.sig;
          res.best_row = (int64_t)row;
        }
      }
    }
    res.next.optimistic_slot = opt_att;
    if (t != FOLD_NONE) {  // the row applied: store.best_valid_update = None (:553)
      has = false;
      b_key = 0; b_att = 0; b_sig = 0;
      res.best_row = -1;
    }
    res.next.has_best = has ? 1u : 0u;
    res.next.best_key0 = has ? b_key : 0u;
    res.next.best_att = has ? b_att : 0;
    res.next.best_sig = has ? b_sig : 0;
    res.rows_consumed = t != FOLD_NONE ? (uint64_t)t + 1 : (uint64_t)n;
    res.apply_row = t != FOLD_NONE ? (int64_t)rows(t) : -1;
    *(FoldResult*)out = res;
  }
}
// the whole batch as one store's rows (F_fold)
LCV_FN void item_fold_team(uint32_t lane, uint32_t r, uint32_t* lds, const Work& W, const FoldState& in,
                           uint64_t store_fin_slot, uint32_t next_known, uint32_t n) {
  item_fold_rows(lane, r, lds, W, FoldRowsAll{}, in, store_fin_slot, next_known, n, W.fold_out);
}

// The fold of a store-table batch, store by store (lcv_validate_stores_fold): the host groups the batch's rows by
// store_index into segments — seg_store[g] the store row, seg_row[seg_off[g] .. seg_off[g + 1]) its batch rows in
// ascending order — and gathers the present stores' fold states; team g folds segment g against store row
// seg_store[g] of the table and writes batch row numbers to out + g * FOLD_RESULT_BYTES.
struct FoldSegDev {
  const uint32_t* seg_store;  // [nseg] distinct store rows present, ascending
  const uint32_t* seg_off;    // [nseg + 1]
  const uint32_t* seg_row;    // [n]
  const uint8_t* in;          // [nseg][48] FoldState of store seg_store[g] (16-byte aligned)
  uint8_t* out;               // [nseg][FOLD_RESULT_BYTES]
};
LCV_FN void fold_state_ld(FoldState& s, const uint8_t* base, size_t g) {
  const uint8_t* p = base + sizeof(FoldState) * g;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = (const uint4*)p;  // three 16-byte loads
  const uint4 a = q[0], b = q[1], c = q[2];
  s.optimistic_slot = (uint64_t)a.x | ((uint64_t)a.y << 32);
  s.previous_max = (uint64_t)a.z | ((uint64_t)a.w << 32);
  s.current_max = (uint64_t)b.x | ((uint64_t)b.y << 32);
  s.has_best = b.z; s.best_key0 = b.w;
  s.best_att = (uint64_t)c.x | ((uint64_t)c.y << 32);
  s.best_sig = (uint64_t)c.z | ((uint64_t)c.w << 32);
#else
  memcpy(&s, p, sizeof(FoldState));
#endif
}
LCV_FN void item_fold_seg_team(uint32_t g, uint32_t lane, uint32_t r, uint32_t* lds, const Work& W, const StoreDev& S,
                               const FoldSegDev& G) {
  const uint32_t s = G.seg_store[g], off = G.seg_off[g], len = G.seg_off[g + 1] - off;
  FoldState in;
  fold_state_ld(in, G.in, g);
  item_fold_rows(lane, r, lds, W, FoldRowsSeg{G.seg_row + off}, in, S.fin_slot[s],
                 S.next[s] != STORE_NEXT_UNKNOWN ? 1u : 0u, len, G.out + (size_t)FOLD_RESULT_BYTES * g);
}

}  // namespace lcv
