// lcv_producer.hpp — the producer side on the device (full-node.md): light-client updates and bootstraps derived
// in batches from tables of sparse state / block views (include/lcv.h: lcv_state_views, lcv_block_views).
//   stage 0   hash_tree_root(SyncCommittee) per committee row: F_nsc_team (lcv_items.hpp), as validation runs it
//   stage 1a  item_prod_block, one lane per block view: sync-aggregate root, execution root, the 16-leaf body tree
//             -> BeaconBlockHeader, block root, execution branch (gindex 25)
//   stage 1b  item_prod_state, one lane per state view: the 32-leaf state tree -> state root, the branches of
//             gindices 54, 55 and 105, and the root of latest_block_header with that state root filled in
//   stage 2   item_prod_rows, PROD_TEAM lanes per update: lane 0 runs create_light_client_update's asserts on the
//             stage-1 values (first failing check = reason), then the team gathers the row (about 2.6 KB from the
//             view tables and the stage-1 rows into the 13 columns of a packed batch) in 16-byte accesses
// Every tree is hashed once: an incremental stack builds each layer's nodes in order and the proofs' siblings are
// stored as they complete.  Reference: full-node.md:43-91, :105-121, :138-188, :197-219 (as lcv/producer.py).
#pragma once
#include "lcv_items.hpp"

namespace lcv {

struct ProdStates {
  const uint64_t* slot; const uint8_t* header; const uint64_t* fin_epoch; const uint8_t* fin_root;
  const uint8_t* roots; const uint32_t* cur; const uint32_t* nxt;
};
struct ProdBlocks {
  const uint64_t* slot; const uint64_t* proposer; const uint8_t* parent; const uint8_t* state_root;
  const uint8_t* bits; const uint8_t* sig; const uint8_t* exec; const uint8_t* kind; const uint8_t* roots;
};
struct ProdCases {
  const uint32_t* state; const uint32_t* block; const uint32_t* att_state; const uint32_t* att_block;
  const int32_t* fin_block;
};
// the stage-0 / stage-1 values, one scratch allocation per call.  Block row (272 B): header 112, block root 32,
// execution branch 128.  State row (576 B, 18 chunks): state root, header root, the 5 siblings of leaf 22, the 5
// of leaf 23, the finality branch (epoch chunk + the 5 siblings of leaf 20) — each branch contiguous, so the
// gather copies it as one run.  Rows and pieces are multiples of 16 bytes.
enum {
  PROD_BLK_ROW = 272, PROD_BLK_ROOT = 112, PROD_BLK_BRANCH = 144,
  PROD_ST_ROW = 576, PROD_ST_ROOT = 0, PROD_ST_HDR_ROOT = 32, PROD_ST_CUR = 64, PROD_ST_NXT = 224, PROD_ST_FIN = 384,
  PROD_STATE_FIELDS = 28, PROD_BODY_FIELDS = 12,
};
struct ProdScratch {
  const uint32_t* comm_root;  // [8][pool_cap] HTR(SyncCommittee) of the pool rows (F_nsc_team's W.nsc_root)
  uint32_t pool_cap;
  uint8_t* blk;  // [nb][PROD_BLK_ROW]
  uint8_t* st;   // [ns][PROD_ST_ROW]
};
// the packed batch being written (the columns of BatchDev)
struct ProdOut {
  uint8_t* att_beacon; uint8_t* att_exec; uint8_t* att_branch; uint8_t* fin_beacon; uint8_t* fin_exec;
  uint8_t* fin_branch; uint32_t* nsc_index; uint8_t* nsc_branch; uint8_t* finality_branch; uint8_t* bits;
  uint8_t* sig; uint64_t* sig_slot;
};

// ---- 16-byte moves (the gather's unit): consecutive lanes, consecutive 16-byte words
struct q128 { uint32_t x, y, z, w; };
LCV_FN q128 ld_q128(const uint8_t* p, uint32_t k) {
  q128 r;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 t = ((const uint4*)p)[k];
  r.x = t.x; r.y = t.y; r.z = t.z; r.w = t.w;
#else
  memcpy(&r, p + 16 * (size_t)k, 16);
#endif
  return r;
}
LCV_FN void st_q128(uint8_t* p, uint32_t k, const q128& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  ((uint4*)p)[k] = make_uint4(v.x, v.y, v.z, v.w);
#else
  memcpy(p + 16 * (size_t)k, &v, 16);
#endif
}
// dst[0 .. bytes) = on ? src : 0, the team's lanes striding over the 16-byte words.  blob_mask (an execution
// record of a Capella, pre-Deneb header): bytes 480..487 and 512..519 (blob_gas_used, excess_blob_gas) zeroed
template <uint32_t TEAM>
LCV_FN void team_copy(uint8_t* dst, const uint8_t* src, uint32_t bytes, uint32_t lane, bool on, bool blob_mask = false) {
  for (uint32_t k = lane; k < bytes / 16; k += TEAM) {
    q128 v = {0u, 0u, 0u, 0u};
    if (on) {
      v = ld_q128(src, k);
      if (blob_mask && (k == 30u || k == 32u)) v.x = v.y = 0u;
    }
    st_q128(dst, k, v);
  }
}

LCV_FN void st_le64(uint8_t* p, uint64_t v) {
  *(uint32_t*)p = (uint32_t)v;
  *(uint32_t*)(p + 4) = (uint32_t)(v >> 32);
}

// hash_tree_root(BeaconBlockHeader) of its five fields
LCV_FN void htr_beacon_fields(h256& root, uint64_t slot, uint64_t proposer, const h256& parent, const h256& state,
                              const h256& body) {
  h256 a, b, z, n0, n1, n2;
  u64_chunk(a, slot);
  u64_chunk(b, proposer);
  hash_pair(n0, a, b);
  hash_pair(n1, parent, state);
  zero_hash(z, 0);
  hash_pair(n2, body, z);
  hash_pair(n0, n0, n1);
  zero_hash(z, 1);
  hash_pair(n2, n2, z);
  hash_pair(root, n0, n2);
}

// ============================================================================ stage 1a: block views
// leaf j (uniform over the lanes) joins the body tree; the level-1 node 5 is a sibling of leaf 9's path
template <int L> LCV_FN void prod_body_push(h256 (&s)[4], h256& node, uint32_t j, uint8_t* branch) {
  if constexpr (L == 1) {
    if ((j >> 1) == 5u) st_chunk(branch + 32, node);
  }
  if constexpr (L >= 3) {
    s[3] = node;  // the left half's root (12 leaves never complete the right half)
  } else {
    if ((j >> L) & 1u) {
      hash_pair(node, s[L], node);
      prod_body_push<L + 1>(s, node, j, branch);
    } else {
      s[L] = node;
    }
  }
}

LCV_FN void item_prod_block(uint32_t b, const ProdBlocks& K, const ProdScratch& X) {
  uint8_t* o = X.blk + (size_t)PROD_BLK_ROW * b;
  uint8_t* branch = o + PROD_BLK_BRANCH;
  const uint32_t kind = K.kind[b];
  h256 agg, er, x, y, z;
  {  // hash_tree_root(SyncAggregate): H(HTR(bits), HTR(signature))
    const uint8_t* bits = K.bits + 64 * (size_t)b;
    const uint8_t* sig = K.sig + 96 * (size_t)b;
    ld_chunk(x, bits);
    ld_chunk(y, bits + 32);
    hash_pair(agg, x, y);
    ld_chunk(x, sig);
    ld_chunk(y, sig + 32);
    hash_pair(x, x, y);
    ld_chunk(y, sig + 64);
    zero_hash(z, 0);
    hash_pair(y, y, z);
    hash_pair(x, x, y);
    hash_pair(agg, agg, x);
  }
  h256_zero(er);
  if (kind != 0u) htr_exec(er, K.exec + (size_t)K_EXEC * b, kind == 2u);
  h256 s[4], node;
  LCV_NOUNROLL for (uint32_t j = 0; j < (uint32_t)PROD_BODY_FIELDS; ++j) {
    if (j == 8u) node = agg;
    else if (j == 9u && kind != 0u) node = er;
    else ld_chunk(node, K.roots + 32 * ((size_t)PROD_BODY_FIELDS * b + j));
    if (j == 8u) st_chunk(branch, node);  // leaf 9's neighbour
    prod_body_push<0>(s, node, j, branch);
  }
  // leaves 12..15 are empty: the level-2 node 3 is the zero subtree
  zero_hash(z, 2);
  st_chunk(branch + 64, z);
  hash_pair(x, s[2], z);
  st_chunk(branch + 96, s[3]);
  hash_pair(node, s[3], x);  // body root
  const uint64_t slot = K.slot[b], proposer = K.proposer[b];
  st_le64(o, slot);
  st_le64(o + 8, proposer);
  ld_chunk(x, K.parent + 32 * (size_t)b);
  ld_chunk(y, K.state_root + 32 * (size_t)b);
  st_chunk(o + 16, x);
  st_chunk(o + 48, y);
  st_chunk(o + 80, node);
  h256 root;
  htr_beacon_fields(root, slot, proposer, x, y, node);
  st_chunk(o + PROD_BLK_ROOT, root);
}

// ============================================================================ stage 1b: state views
template <int L> LCV_FN void prod_state_push(h256 (&s)[5], h256& node, uint32_t j, uint8_t* o) {
  if constexpr (L == 1) {
    if ((j >> 1) == 10u) { st_chunk(o + PROD_ST_CUR + 32, node); st_chunk(o + PROD_ST_NXT + 32, node); }
    if ((j >> 1) == 11u) st_chunk(o + PROD_ST_FIN + 64, node);
  }
  if constexpr (L == 2) {
    if ((j >> 2) == 4u) {
      st_chunk(o + PROD_ST_CUR + 64, node); st_chunk(o + PROD_ST_NXT + 64, node); st_chunk(o + PROD_ST_FIN + 96, node);
    }
  }
  if constexpr (L >= 4) {
    s[4] = node;  // the left half's root (28 leaves never complete the right half)
  } else {
    if ((j >> L) & 1u) {
      hash_pair(node, s[L], node);
      prod_state_push<L + 1>(s, node, j, o);
    } else {
      s[L] = node;
    }
  }
}

LCV_FN void item_prod_state(uint32_t t, const ProdStates& S, const ProdScratch& X) {
  uint8_t* o = X.st + (size_t)PROD_ST_ROW * t;
  const uint8_t* hdr = S.header + (size_t)K_BEACON * t;
  const uint64_t epoch = S.fin_epoch[t];
  h256 s[5], node, x, z;
  LCV_NOUNROLL for (uint32_t j = 0; j < (uint32_t)PROD_STATE_FIELDS; ++j) {
    if (j == 2u) {
      u64_chunk(node, S.slot[t]);
    } else if (j == 4u) {
      htr_beacon(node, hdr);  // latest_block_header as the state holds it
    } else if (j == 20u) {    // Checkpoint(epoch, root)
      u64_chunk(x, epoch);
      ld_chunk(node, S.fin_root + 32 * (size_t)t);
      hash_pair(node, x, node);
    } else if (j == 22u) {
      soa_ld_h256(node, X.comm_root, X.pool_cap, S.cur[t]);
    } else if (j == 23u) {
      soa_ld_h256(node, X.comm_root, X.pool_cap, S.nxt[t]);
    } else {
      ld_chunk(node, S.roots + 32 * ((size_t)PROD_STATE_FIELDS * t + j));
    }
    if (j == 21u) st_chunk(o + PROD_ST_FIN + 32, node);
    if (j == 22u) st_chunk(o + PROD_ST_NXT, node);
    if (j == 23u) st_chunk(o + PROD_ST_CUR, node);
    prod_state_push<0>(s, node, j, o);
  }
  // leaves 28..31 are empty: s[2] is the level-2 node 6, its neighbour the zero subtree
  zero_hash(z, 2);
  hash_pair(x, s[2], z);  // level-3 node 3
  st_chunk(o + PROD_ST_CUR + 96, x); st_chunk(o + PROD_ST_NXT + 96, x); st_chunk(o + PROD_ST_FIN + 128, x);
  hash_pair(x, s[3], x);  // level-4 node 1
  st_chunk(o + PROD_ST_CUR + 128, s[4]); st_chunk(o + PROD_ST_NXT + 128, s[4]); st_chunk(o + PROD_ST_FIN + 160, s[4]);
  hash_pair(node, s[4], x);  // hash_tree_root(state)
  st_chunk(o + PROD_ST_ROOT, node);
  u64_chunk(x, epoch);
  st_chunk(o + PROD_ST_FIN, x);
  // hash_tree_root(latest_block_header) with state_root = hash_tree_root(state) (full-node.md:147-148)
  h256 parent, body, root;
  ld_chunk(parent, hdr + 16);
  ld_chunk(body, hdr + 80);
  htr_beacon_fields(root, ld_le64(hdr), ld_le64(hdr + 8), parent, node, body);
  st_chunk(o + PROD_ST_HDR_ROOT, root);
}

// ============================================================================ stage 2: decide, then gather
// 16 lanes per row, 4 rows per wave: a row is ten runs of 64..832 bytes (4..52 16-byte words), six of them at most
// 12 words, so a 16-lane team moves most runs in one pass with consecutive lanes on consecutive words (256 bytes,
// two whole cache lines per access) and the wave keeps four rows' runs in flight; a 64-lane team would idle on three
// quarters or more of its lanes in those six runs.  DESIGN.md §3.8.
enum { PROD_TEAM = 16, PROD_ROUNDS = 2, PROD_LDS = 4 };
enum : uint32_t {
  PF_ATT_EXEC = 1u, PF_ATT_MASK = 2u, PF_NSC = 4u, PF_FIN_HDR = 8u, PF_FIN_EXEC = 16u, PF_FIN_MASK = 32u,
  PF_FIN_BRANCH = 64u,
};

LCV_FN bool chunk_eq(const uint8_t* a, const uint8_t* b) {
  uint32_t d = 0;
  LCV_UNROLL for (int k = 0; k < 8; ++k) d |= ((const uint32_t*)a)[k] ^ ((const uint32_t*)b)[k];
  return d == 0;
}
// block_to_light_client_header's fork cases for block b: false = the payload is missing (ValueError)
LCV_FN bool prod_header_flags(uint32_t b, const ProdBlocks& K, const NetConfig& cfg, bool& exec, bool& mask) {
  const uint64_t epoch = epoch_of_slot(K.slot[b], cfg);
  exec = epoch >= cfg.fork_epoch[FORK_CAPELLA];
  mask = exec && epoch < cfg.fork_epoch[FORK_DENEB];
  return !(exec && K.kind[b] == 0u);
}

// create_light_client_update's checks in evaluation order (full-node.md:143-174) -> reason, and what the row holds
LCV_FN uint32_t prod_decide(uint32_t i, const ProdStates& S, const ProdBlocks& K, const ProdCases& C,
                            const ProdScratch& X, const NetConfig& cfg, uint32_t kind, uint32_t& flags) {
  const uint32_t st = C.state[i], bk = C.block[i], as = C.att_state[i], ab = C.att_block[i];
  const int32_t fb = C.fin_block[i];
  flags = 0;
  if (epoch_of_slot(S.slot[as], cfg) < cfg.fork_epoch[FORK_ALTAIR]) return 1;
  if (popcount_bits(K.bits + 64 * (size_t)bk) < 1u) return 2;
  if (S.slot[st] != ld_le64(S.header + (size_t)K_BEACON * st)) return 3;
  const uint8_t* st_row = X.st + (size_t)PROD_ST_ROW * st;
  const uint8_t* as_row = X.st + (size_t)PROD_ST_ROW * as;
  const uint8_t* ab_row = X.blk + (size_t)PROD_BLK_ROW * ab;
  if (!chunk_eq(st_row + PROD_ST_HDR_ROOT, X.blk + (size_t)PROD_BLK_ROW * bk + PROD_BLK_ROOT)) return 4;
  if (S.slot[as] != ld_le64(S.header + (size_t)K_BEACON * as)) return 5;
  if (!chunk_eq(as_row + PROD_ST_HDR_ROOT, ab_row + PROD_BLK_ROOT) ||
      !chunk_eq(ab_row + PROD_BLK_ROOT, K.parent + 32 * (size_t)bk))
    return 6;
  bool exec, mask;
  if (!prod_header_flags(ab, K, cfg, exec, mask)) return 7;
  uint32_t f = (exec ? PF_ATT_EXEC : 0u) | (mask ? PF_ATT_MASK : 0u);
  if (period_of_slot(K.slot[ab], cfg) == period_of_slot(K.slot[bk], cfg)) f |= PF_NSC;
  if (fb >= 0) {
    const uint8_t* fin_root = S.fin_root + 32 * (size_t)as;
    if (K.slot[fb] != 0u) {
      if (!prod_header_flags((uint32_t)fb, K, cfg, exec, mask)) return 8;
      if (!chunk_eq(X.blk + (size_t)PROD_BLK_ROW * fb + PROD_BLK_ROOT, fin_root)) return 9;
      f |= PF_FIN_HDR | (exec ? PF_FIN_EXEC : 0u) | (mask ? PF_FIN_MASK : 0u);
    } else {
      if (!bytes_all_zero(fin_root, 8)) return 10;
    }
    f |= PF_FIN_BRANCH;
  }
  // create_light_client_finality_update / _optimistic_update keep a subset of the update's fields
  if (kind >= 1u) f &= ~(uint32_t)PF_NSC;
  if (kind >= 2u) f &= ~(uint32_t)(PF_FIN_HDR | PF_FIN_EXEC | PF_FIN_MASK | PF_FIN_BRANCH);
  flags = f;
  return 0;
}

// one LightClientHeader: beacon, execution record, execution branch of block view b (on), or the empty header
template <uint32_t TEAM>
LCV_FN void team_header(uint8_t* beacon, uint8_t* exec, uint8_t* branch, size_t row, uint32_t b, const ProdBlocks& K,
                        const ProdScratch& X, uint32_t lane, bool on, bool with_exec, bool mask) {
  const uint8_t* src = X.blk + (size_t)PROD_BLK_ROW * b;
  team_copy<TEAM>(beacon + (size_t)K_BEACON * row, src, K_BEACON, lane, on);
  team_copy<TEAM>(exec + (size_t)K_EXEC * row, K.exec + (size_t)K_EXEC * b, K_EXEC, lane, on && with_exec, mask);
  team_copy<TEAM>(branch + (size_t)K_EXEC_BRANCH * row, src + PROD_BLK_BRANCH, K_EXEC_BRANCH, lane, on && with_exec);
}

LCV_FN void item_prod_rows(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, const ProdStates& S,
                           const ProdBlocks& K, const ProdCases& C, const ProdScratch& X, const ProdOut& O,
                           const NetConfig& cfg, uint32_t kind, uint32_t ncomm, uint8_t* reason_out) {
  if (r == 0) {
    if (lane == 0) {
      uint32_t flags;
      const uint32_t reason = prod_decide(i, S, K, C, X, cfg, kind, flags);
      lds[0] = reason;
      lds[1] = flags;
      reason_out[i] = (uint8_t)reason;
    }
    return;
  }
  const bool ok = lds[0] == 0u;
  const uint32_t f = lds[1];
  const uint32_t bk = C.block[i], as = C.att_state[i], ab = C.att_block[i];
  const int32_t fb = C.fin_block[i];
  const uint32_t fbu = fb >= 0 ? (uint32_t)fb : 0u;
  const uint8_t* as_row = X.st + (size_t)PROD_ST_ROW * as;
  team_header<PROD_TEAM>(O.att_beacon, O.att_exec, O.att_branch, i, ab, K, X, lane, ok, (f & PF_ATT_EXEC) != 0u,
                         (f & PF_ATT_MASK) != 0u);
  team_header<PROD_TEAM>(O.fin_beacon, O.fin_exec, O.fin_branch, i, fbu, K, X, lane, (f & PF_FIN_HDR) != 0u,
                         (f & PF_FIN_EXEC) != 0u, (f & PF_FIN_MASK) != 0u);
  team_copy<PROD_TEAM>(O.nsc_branch + (size_t)K_NSC_BRANCH * i, as_row + PROD_ST_NXT, K_NSC_BRANCH, lane, (f & PF_NSC) != 0u);
  team_copy<PROD_TEAM>(O.finality_branch + (size_t)K_FIN_BRANCH * i, as_row + PROD_ST_FIN, K_FIN_BRANCH, lane,
                       (f & PF_FIN_BRANCH) != 0u);
  team_copy<PROD_TEAM>(O.bits + 64 * (size_t)i, K.bits + 64 * (size_t)bk, 64, lane, ok);
  team_copy<PROD_TEAM>(O.sig + 96 * (size_t)i, K.sig + 96 * (size_t)bk, 96, lane, ok);
  if (lane == 0) {
    O.nsc_index[i] = (f & PF_NSC) ? S.nxt[as] : ncomm;
    O.sig_slot[i] = ok ? K.slot[bk] : 0u;
  }
}

// rows[i] of a resident batch -> row i of another (lcv_batch_download's row list), the same 16-lane gather
LCV_FN void item_prod_pick(uint32_t i, uint32_t lane, const BatchDev& B, const uint32_t* rows, const ProdOut& O) {
  const size_t s = rows[i];
  team_copy<PROD_TEAM>(O.att_beacon + (size_t)K_BEACON * i, B.att_beacon + (size_t)K_BEACON * s, K_BEACON, lane, true);
  team_copy<PROD_TEAM>(O.att_exec + (size_t)K_EXEC * i, B.att_exec + (size_t)K_EXEC * s, K_EXEC, lane, true);
  team_copy<PROD_TEAM>(O.att_branch + (size_t)K_EXEC_BRANCH * i, B.att_branch + (size_t)K_EXEC_BRANCH * s, K_EXEC_BRANCH, lane, true);
  team_copy<PROD_TEAM>(O.fin_beacon + (size_t)K_BEACON * i, B.fin_beacon + (size_t)K_BEACON * s, K_BEACON, lane, true);
  team_copy<PROD_TEAM>(O.fin_exec + (size_t)K_EXEC * i, B.fin_exec + (size_t)K_EXEC * s, K_EXEC, lane, true);
  team_copy<PROD_TEAM>(O.fin_branch + (size_t)K_EXEC_BRANCH * i, B.fin_branch + (size_t)K_EXEC_BRANCH * s, K_EXEC_BRANCH, lane, true);
  team_copy<PROD_TEAM>(O.nsc_branch + (size_t)K_NSC_BRANCH * i, B.nsc_branch + (size_t)K_NSC_BRANCH * s, K_NSC_BRANCH, lane, true);
  team_copy<PROD_TEAM>(O.finality_branch + (size_t)K_FIN_BRANCH * i, B.finality_branch + (size_t)K_FIN_BRANCH * s, K_FIN_BRANCH, lane, true);
  team_copy<PROD_TEAM>(O.bits + 64 * (size_t)i, B.bits + 64 * s, 64, lane, true);
  team_copy<PROD_TEAM>(O.sig + 96 * (size_t)i, B.sig + 96 * s, 96, lane, true);
  if (lane == 0) {
    O.nsc_index[i] = B.nsc_index[s];
    O.sig_slot[i] = B.sig_slot[s];
  }
}

// create_light_client_bootstrap (full-node.md:105-121) of (state_idx[i], block_idx[i]): reason 1 :107, 2 :109,
// 3 :112, 4 missing payload; the columns lcv_bootstrap_check_batch takes, the committee as a pool row
struct ProdBootOut {
  uint8_t* beacon; uint8_t* exec; uint8_t* branch; uint32_t* committee_index; uint8_t* committee_branch;
  uint8_t* reason;
};
LCV_FN void item_prod_boot(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, const ProdStates& S,
                           const ProdBlocks& K, const uint32_t* state_idx, const uint32_t* block_idx,
                           const ProdScratch& X, const ProdBootOut& O, const NetConfig& cfg, uint32_t ncomm) {
  const uint32_t st = state_idx[i], bk = block_idx[i];
  const uint8_t* st_row = X.st + (size_t)PROD_ST_ROW * st;
  if (r == 0) {
    if (lane == 0) {
      bool exec = false, mask = false;
      uint32_t reason = 0;
      if (epoch_of_slot(S.slot[st], cfg) < cfg.fork_epoch[FORK_ALTAIR]) reason = 1;
      else if (S.slot[st] != ld_le64(S.header + (size_t)K_BEACON * st)) reason = 2;
      else if (!chunk_eq(st_row + PROD_ST_HDR_ROOT, X.blk + (size_t)PROD_BLK_ROW * bk + PROD_BLK_ROOT)) reason = 3;
      else if (!prod_header_flags(bk, K, cfg, exec, mask)) reason = 4;
      lds[0] = reason;
      lds[1] = (exec ? PF_ATT_EXEC : 0u) | (mask ? PF_ATT_MASK : 0u);
      O.reason[i] = (uint8_t)reason;
    }
    return;
  }
  const bool ok = lds[0] == 0u;
  const uint32_t f = lds[1];
  team_header<PROD_TEAM>(O.beacon, O.exec, O.branch, i, bk, K, X, lane, ok, (f & PF_ATT_EXEC) != 0u, (f & PF_ATT_MASK) != 0u);
  team_copy<PROD_TEAM>(O.committee_branch + (size_t)K_NSC_BRANCH * i, st_row + PROD_ST_CUR, K_NSC_BRANCH, lane, ok);
  if (lane == 0) O.committee_index[i] = ok ? S.cur[st] : ncomm;
}

}  // namespace lcv

// ---- one functor per kernel (LCV_HD: __device__ in lcv_k_prod.hip, empty in the host simulation)
struct F_prod_block {
  lcv::ProdBlocks K; lcv::ProdScratch X;
  LCV_HD void operator()(uint32_t b) const { lcv::item_prod_block(b, K, X); }
};
struct F_prod_state {
  lcv::ProdStates S; lcv::ProdScratch X;
  LCV_HD void operator()(uint32_t t) const { lcv::item_prod_state(t, S, X); }
};
struct F_prod_rows {
  lcv::ProdStates S; lcv::ProdBlocks K; lcv::ProdCases C; lcv::ProdScratch X; lcv::ProdOut O; lcv::NetConfig cfg;
  uint32_t kind, ncomm; uint8_t* reason;
  static constexpr uint32_t TEAM = lcv::PROD_TEAM, LDS_WORDS = lcv::PROD_LDS, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return lcv::PROD_ROUNDS; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, uint32_t*) const {
    lcv::item_prod_rows(i, lane, r, lds, S, K, C, X, O, cfg, kind, ncomm, reason);
  }
};
struct F_prod_pick {
  lcv::BatchDev B; const uint32_t* rows; lcv::ProdOut O;
  static constexpr uint32_t TEAM = lcv::PROD_TEAM, LDS_WORDS = 1, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return 1; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t, uint32_t*, uint32_t*) const {
    lcv::item_prod_pick(i, lane, B, rows, O);
  }
};
struct F_prod_boot {
  lcv::ProdStates S; lcv::ProdBlocks K; const uint32_t* state_idx; const uint32_t* block_idx; lcv::ProdScratch X;
  lcv::ProdBootOut O; lcv::NetConfig cfg; uint32_t ncomm;
  static constexpr uint32_t TEAM = lcv::PROD_TEAM, LDS_WORDS = lcv::PROD_LDS, SHARED_WORDS = 0;
  LCV_HD uint32_t rounds() const { return lcv::PROD_ROUNDS; }
  LCV_HD void operator()(uint32_t i, uint32_t lane, uint32_t r, uint32_t* lds, uint32_t*) const {
    lcv::item_prod_boot(i, lane, r, lds, S, K, state_idx, block_idx, X, O, cfg, ncomm);
  }
};
