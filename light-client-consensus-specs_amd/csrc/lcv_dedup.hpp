// lcv_dedup.hpp — device side of the deduplicated BLS half (lcv_set_dedup, include/lcv.h "Deduplicated
// signatures").  The host groups the rows of a chunk into items (lcv_dedup_plan.hpp: rep[row] = item, urow[item] =
// its first row); the pre-checks run over all n rows as ever; F_dedup_gather then writes the BLS inputs of items
// 0 .. m-1 into compact columns, the BLS stages run unchanged over those m items (a BatchDev view of the compact
// columns, a Work view whose comm_id is the compact one), and F_verdict_dedup gives every row its item's verdict.
//
// Classing a resident batch where it lies (lcv_batch_classify): F_dedup_key, one team per row, folds the row's tuple
// (attested beacon 112 B, bits 64 B, signature 96 B: 17 aligned 16-byte words; signature_slot) into one 64-bit key; the
// host groups the keys (dedup_group) and F_dedup_confirm, one team per listed pair of rows, compares the two tuples'
// 280 bytes in full.  The key only decides which rows are compared, never that two rows are equal.  No round reads
// LDS that the same round writes.
#pragma once
#include "lcv_producer.hpp"  // team_copy

namespace lcv {

// the slot's scratch (lcv_driver.inc ensure_dedup): per item the four batch columns the BLS stages read and the
// committee id F_pre chose for the item's first row; per row the grouping of a resident batch's chunk
struct DedupDev {
  uint8_t* att_beacon;  // [cap][112]
  uint64_t* sig_slot;   // [cap]
  uint8_t* bits;        // [cap][64]
  uint8_t* sig;         // [cap][96]
  uint32_t* comm_id;    // [cap]  W.comm_id[urow[u]]: an array of its own (urow[u] >= u: gathering in place would race)
  uint32_t* rep;        // [cap]  row -> item
  uint32_t* urow;       // [cap]  item -> first row
};

// item u <- row urow[u], DEDUP_TEAM lanes striding over the 16-byte words of the three byte columns (17 words);
// signature_slot as two 4-byte words and the committee id as one, on lanes of their own
enum { DEDUP_TEAM = 16 };
LCV_FN void item_dedup_gather(uint32_t u, uint32_t lane, const BatchDev& B, const Work& W, const uint32_t* urow,
                              const DedupDev& D) {
  const size_t s = urow[u];
  team_copy<DEDUP_TEAM>(D.att_beacon + (size_t)K_BEACON * u, B.att_beacon + (size_t)K_BEACON * s, K_BEACON, lane, true);
  team_copy<DEDUP_TEAM>(D.bits + 64 * (size_t)u, B.bits + 64 * s, 64, lane, true);
  team_copy<DEDUP_TEAM>(D.sig + 96 * (size_t)u, B.sig + 96 * s, 96, lane, true);
  if (lane >= 8u && lane < 10u) ((uint32_t*)(D.sig_slot + u))[lane - 8u] = ((const uint32_t*)(B.sig_slot + s))[lane - 8u];
  if (lane == 10u) D.comm_id[u] = W.comm_id[s];
}

// item_verdict for row i with the BLS flags of its item rep[i]; the pre-check reason is the row's own
LCV_FN void item_verdict_dedup(uint32_t i, const Work& W, const uint32_t* rep) {
  uint32_t reason = W.pre_reason[i];
  if (reason == 0) {
    const uint32_t u = rep[i];
    const bool ok = W.agg_status[u] == PT_OK && W.sig_status[u] != PT_BAD && W.pair_ok[u] != 0;
    reason = ok ? 0 : 14;  // :464
  }
  W.reason[i] = (uint8_t)reason;
  W.verdict[i] = reason == 0 ? 1 : 0;
}

// ---- the class of a row.  Tuple word w of row s: 0..6 the attested beacon header, 7..10 the bits, 11..16 the signature
enum { DEDUP_KEY_WORDS = 17, DEDUP_KEY_LDS = 2 * DEDUP_TEAM, DEDUP_CONFIRM_LDS = DEDUP_TEAM };
LCV_FN uint64_t dedup_key_mix(uint64_t h, uint64_t x) {  // (dec_mix's shape)
  h = (h ^ x) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
constexpr uint64_t DEDUP_KEY_SEED = 0x6c63765f636c6173ull;
LCV_FN q128 dedup_tuple_word(const BatchDev& B, size_t s, uint32_t w) {
  if (w < 7u) return ld_q128(B.att_beacon + (size_t)K_BEACON * s, w);
  if (w < 11u) return ld_q128(B.bits + 64 * s, w - 7u);
  return ld_q128(B.sig + 96 * s, w - 11u);
}
// round 0: lane l folds (w, word w) for w = l, l + 16 and, lane 1, signature_slot under index 17, into a value kept in
// its own two LDS words; round 1: lane 0 combines the lanes' values in lane order and stores the row's key
LCV_FN void item_dedup_key(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, const BatchDev& B, uint64_t* key) {
  if (r == 0) {
    uint64_t h = dedup_key_mix(DEDUP_KEY_SEED, lane);
    for (uint32_t w = lane; w < (uint32_t)DEDUP_KEY_WORDS; w += DEDUP_TEAM) {
      const q128 v = dedup_tuple_word(B, i, w);
      h = dedup_key_mix(h, w);
      h = dedup_key_mix(h, (uint64_t)v.x | ((uint64_t)v.y << 32));
      h = dedup_key_mix(h, (uint64_t)v.z | ((uint64_t)v.w << 32));
    }
    if (lane == 1u) {
      h = dedup_key_mix(h, (uint64_t)DEDUP_KEY_WORDS);
      h = dedup_key_mix(h, B.sig_slot[i]);
    }
    lds[2u * lane] = (uint32_t)h;
    lds[2u * lane + 1u] = (uint32_t)(h >> 32);
    return;
  }
  if (lane == 0) {
    uint64_t h = 0;
    LCV_NOUNROLL for (uint32_t l = 0; l < (uint32_t)DEDUP_TEAM; ++l)
      h = dedup_key_mix(h, (uint64_t)lds[2u * l] | ((uint64_t)lds[2u * l + 1u] << 32));
    key[i] = h;
  }
}
// pair k = rows (pairs[2k], pairs[2k + 1]) of B, both below B.n (the host has checked): differ[k] = 1 where the tuples
// differ in any of their 280 bytes.  F_sc_confirm over batch columns
LCV_FN void item_dedup_confirm(uint32_t k, uint32_t lane, uint32_t r, uint32_t* lds, const BatchDev& B,
                               const uint32_t* pairs, uint32_t* differ) {
  if (r == 0) {
    const size_t a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
    uint32_t d = 0;
    for (uint32_t w = lane; w < (uint32_t)DEDUP_KEY_WORDS; w += DEDUP_TEAM) {
      const q128 x = dedup_tuple_word(B, a, w), y = dedup_tuple_word(B, b, w);
      d |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    if (lane == 1u) d |= B.sig_slot[a] != B.sig_slot[b] ? 1u : 0u;
    lds[lane] = d;
    return;
  }
  if (lane == 0) {
    uint32_t d = 0;
    LCV_NOUNROLL for (uint32_t l = 0; l < (uint32_t)DEDUP_TEAM; ++l) d |= lds[l];
    differ[k] = d ? 1u : 0u;
  }
}

}  // namespace lcv

struct F_dedup_key {
  lcv::BatchDev B; uint64_t* key;
  static constexpr uint32_t TEAM = lcv::DEDUP_TEAM, LDS_WORDS = lcv::DEDUP_KEY_LDS, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return 2; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, uint32_t*) const {
    lcv::item_dedup_key(i, lane, r, lds, B, key);
  }
};
struct F_dedup_confirm {
  lcv::BatchDev B; const uint32_t* pairs; uint32_t* differ;
  static constexpr uint32_t TEAM = lcv::DEDUP_TEAM, LDS_WORDS = lcv::DEDUP_CONFIRM_LDS, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return 2; }
  LCV_HD void operator()(uint32_t k, uint32_t lane, uint32_t r, uint32_t* lds, uint32_t*) const {
    lcv::item_dedup_confirm(k, lane, r, lds, B, pairs, differ);
  }
};
struct F_dedup_gather {
  lcv::BatchDev B; lcv::Work W; const uint32_t* urow; lcv::DedupDev D;
  static constexpr uint32_t TEAM = lcv::DEDUP_TEAM, LDS_WORDS = 1, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return 1; }
  LCV_HD void operator()(uint32_t u, uint32_t lane, uint32_t, uint32_t*, uint32_t*) const {
    lcv::item_dedup_gather(u, lane, B, W, urow, D);
  }
};
struct F_verdict_dedup {
  lcv::Work W; const uint32_t* rep;
  LCV_HD void operator()(uint32_t i) const { lcv::item_verdict_dedup(i, W, rep); }
};
