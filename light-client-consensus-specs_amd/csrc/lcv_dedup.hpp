// lcv_dedup.hpp — device side of the deduplicated BLS half (lcv_set_dedup, include/lcv.h "Deduplicated
// signatures").  The host groups the rows of a chunk into items (lcv_dedup_plan.hpp: rep[row] = item, urow[item] =
// its first row); the pre-checks run over all n rows as ever; F_dedup_gather then writes the BLS inputs of items
// 0 .. m-1 into compact columns, the BLS stages run unchanged over those m items (a BatchDev view of the compact
// columns, a Work view whose comm_id is the compact one), and F_verdict_dedup gives every row its item's verdict.
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

}  // namespace lcv

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
