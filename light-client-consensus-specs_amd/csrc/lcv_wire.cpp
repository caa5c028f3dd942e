// SSZ wire decode of light-client messages into the packed SoA rows of include/lcv.h, on the host.
//
// The containers, their wire order and the rule for what is malformed are lcv_wire_layout.hpp's (the device decoder
// and encoder read the same tables): decoding is strict, as upstream SSZ deserialisation is, and a malformed message
// yields status 1 and an all-zero row.  This file maps the layout's columns to the columns of a batch (or to a
// bootstrap's outputs) and walks the tables over one message.
//
// Finality / optimistic updates become the LightClientUpdate the reference builds from them
// (sync-protocol.md:563-571 / :582-590): default next_sync_committee, zero next-committee branch, and for optimistic
// updates a default finalized header and zero finality branch.  The row of an Altair-format message is the Capella
// upgrade of its data (upgrade_lc_header_to_capella: empty execution and branch).
//
// Distinct next_sync_committee values are deduplicated by content (the device computes HTR(SyncCommittee) once per
// pool row): pool_src[k] = byte offset in `buf` of pool row k's first occurrence, or UINT64_MAX for SyncCommittee()
// (all zero).  Pure host code, no device work.
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/lcv.h"
#include "lcv_dedup_plan.hpp"
#include "lcv_wire_layout.hpp"

namespace {

using namespace lcv;

inline uint32_t rd32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

// where one message's pieces go: p[column][part of a header's columns], null for a piece that is not stored
struct Dest { uint8_t* p[WC_COLS][WH_PARTS]; };
constexpr uint32_t kColBytes[WC_COLS][WH_PARTS] = {
    {K_BEACON, K_EXEC, K_EXEC_BRANCH}, {K_SC}, {K_NSC_BRANCH}, {K_BEACON, K_EXEC, K_EXEC_BRANCH}, {K_FIN_BRANCH}, {K_BITS}, {K_SIG}, {8}};

// row i of a batch (its committee goes to the pool, by content: no column of the row)
Dest row_of(const lcv_update_batch* b, uint64_t i) {
  const void* col[WC_COLS][WH_PARTS] = {
      {b->attested.beacon, b->attested.execution, b->attested.exec_branch}, {}, {b->nsc_branch},
      {b->finalized.beacon, b->finalized.execution, b->finalized.exec_branch}, {b->finality_branch}, {b->sync_bits},
      {b->sync_signature}, {b->signature_slot}};
  Dest d;
  for (int c = 0; c < WC_COLS; ++c)
    for (int h = 0; h < WH_PARTS; ++h)
      d.p[c][h] = col[c][h] ? static_cast<uint8_t*>(const_cast<void*>(col[c][h])) + i * kColBytes[c][h] : nullptr;
  return d;
}

// Decodes one message into d, which is left all zero if the message is malformed; *committee = the offset within the
// message of its committee (the kinds that carry one)
bool decode_msg(const uint8_t* p, uint64_t len, uint32_t kind, uint32_t fork, const Dest& d, uint64_t* committee) {
  for (int c = 0; c < WC_COLS; ++c)
    for (int h = 0; h < WH_PARTS; ++h)
      if (d.p[c][h]) std::memset(d.p[c][h], 0, kColBytes[c][h]);
  const WirePlan plan = wire_accept(kind, fork, len, [p](uint32_t o) { return rd32(p + o); });
  if (plan.status) return false;
  auto seg = [&](uint32_t col, uint32_t part, uint32_t rec, uint32_t o, uint32_t n) {
    if (col == WC_COMMITTEE) *committee = o;
    if (d.p[col][part]) std::memcpy(d.p[col][part] + rec, p + o, n);
  };
  auto put = [](uint32_t, uint32_t) {};  // (the offsets were wire_accept's to check)
  auto header = [&](uint32_t col, uint32_t o, uint32_t elen) {
    wire_walk_header(col, o, fork == WIRE_DENEB, elen, seg, put);
    if (d.p[col][WH_EXEC]) std::memcpy(d.p[col][WH_EXEC] + K_EXEC_EXTRALEN_OFF, &elen, 4);
  };
  wire_walk_fixed(kind, fork == WIRE_ALTAIR, false, 0u, 0u, seg, put, [](uint32_t, uint32_t, uint32_t) { return false; });  // (columns apart)
  if (fork == WIRE_ALTAIR) return true;
  header(WC_ATT, plan.att_off, plan.elen_att);
  if (wire_has(WC_FIN, kind)) header(WC_FIN, plan.fin_off, plan.elen_fin);
  return true;
}

// Dedup key of a committee: a hash of its first pubkey and its aggregate_pubkey (96 sampled bytes);
// every key hit is confirmed by a full 24,624-byte compare, so the sample only has to spread rows.
uint64_t committee_key(const uint8_t* p) {
  uint64_t h = 0x9e3779b97f4a7c15ull;
  auto mix = [&](const uint8_t* q) {
    for (int k = 0; k < 48; k += 8) {
      uint64_t w;
      std::memcpy(&w, q + k, 8);
      h = (h ^ w) * 0xff51afd7ed558ccdull;
      h ^= h >> 29;
    }
  };
  mix(p);
  mix(p + K_SC - 48);
  return h;
}

bool all_zero(const uint8_t* p, uint64_t n) {  // n multiple of 8
  for (uint64_t k = 0; k < n; k += 512) {
    uint64_t acc = 0;
    const uint64_t e = k + 512 < n ? k + 512 : n;
    for (uint64_t j = k; j < e; j += 8) {
      uint64_t w;
      std::memcpy(&w, p + j, 8);
      acc |= w;
    }
    if (acc) return false;
  }
  return true;
}

// rows are independent: split [0, n) over host threads (the batch path; small batches stay inline)
template <class Fn> void parallel_rows(uint64_t n, Fn fn) {
  unsigned t = std::thread::hardware_concurrency();
  t = t < 1 ? 1 : (t > 16 ? 16 : t);
  if (n < 1024 || t == 1) { fn(0, n); return; }
  std::vector<std::thread> pool;
  const uint64_t step = (n + t - 1) / t;
  for (unsigned k = 0; k < t; ++k) {
    const uint64_t lo = k * step, hi = lo + step < n ? lo + step : n;
    if (lo < hi) pool.emplace_back(fn, lo, hi);
  }
  for (auto& th : pool) th.join();
}

}  // namespace

// the batch decode; fork_of(i) gives message i's fork (one per call, or one per Req/Resp chunk)
template <class ForkOf>
static int decode_updates(const uint8_t* buf, const uint64_t* offsets, const uint64_t* lengths, uint64_t n, int kind,
                          ForkOf fork_of, const lcv_update_batch* out, uint64_t* pool_src, uint64_t* npool_out,
                          uint8_t* status) {
  if ((n && (!buf || !offsets || !lengths || !out || !pool_src || !status)) || !npool_out) return LCV_EINVAL;
  if (!wire_kind_ok(kind) || n >= 0xffffffffull) return LCV_EINVAL;  // (rows are numbered in 32 bits: nsc_index)
  if (n) {
    const Dest d = row_of(out, 0);
    for (int c = 0; c < WC_COLS; ++c)
      for (int h = 0; h < WH_PARTS; ++h)
        if (c != WC_COMMITTEE && kColBytes[c][h] && !d.p[c][h]) return LCV_EINVAL;
    if (!out->nsc_index) return LCV_EINVAL;
  }
  constexpr uint64_t kNone = UINT64_MAX;
  constexpr uint32_t none = 0xffffffffu;
  std::vector<uint64_t> csrc(n, kNone), key(n, 0);  // committee offset in buf (kNone: SyncCommittee())
  // 1. decode every row (parallel)
  parallel_rows(n, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; ++i) {
      uint64_t c = kNone;
      const bool ok = decode_msg(buf + offsets[i], lengths[i], (uint32_t)kind, (uint32_t)fork_of(i), row_of(out, i), &c);
      status[i] = ok ? 0 : 1;
      if (ok && c != kNone && !all_zero(buf + offsets[i] + c, K_SC)) {
        csrc[i] = offsets[i] + c;
        key[i] = committee_key(buf + csrc[i]);
      }
    }
  });
  // 2. rep[i] = the first row whose committee equals row i's: the rows grouped by their sampled key alone, then every
  // row but a group's first compared in full with its tentative representative (parallel); rows that differ (distinct
  // committees sharing first and aggregate pubkeys) form the next group under their lowest row
  std::vector<uint32_t> rep(n, none), cand, pending, first;
  for (uint64_t i = 0; i < n; ++i)
    if (csrc[i] != kNone) cand.push_back((uint32_t)i);
  DedupTable table;
  dedup_group(
      (uint32_t)cand.size(), 64, table, [&](uint32_t j) { return key[cand[j]]; }, [](uint32_t, uint32_t) { return true; },
      [&](uint32_t j) { rep[cand[j]] = cand[j]; }, [&](uint32_t a, uint32_t j) { rep[cand[j]] = cand[a]; });
  for (uint32_t r : cand)
    if (rep[r] != r) pending.push_back(r);
  dedup_confirm_groups(rep, pending, [&](const std::vector<uint32_t>& pend, const std::vector<uint32_t>& rp, std::vector<uint32_t>& differ) {
    parallel_rows(pend.size(), [&](uint64_t lo, uint64_t hi) {
      for (uint64_t k = lo; k < hi; ++k) differ[k] = std::memcmp(buf + csrc[pend[k]], buf + csrc[rp[pend[k]]], K_SC) != 0;
    });
    return 0;
  });
  // 3. pool rows in first-occurrence order
  dedup_pool_rows(rep, const_cast<uint32_t*>(out->nsc_index), first);
  for (size_t k = 0; k < first.size(); ++k) pool_src[k] = first[k] == none ? kNone : csrc[first[k]];
  *npool_out = first.size();
  return LCV_OK;
}

extern "C" int lcv_ssz_decode_updates(const uint8_t* buf, const uint64_t* offsets, const uint64_t* lengths,
                                      uint64_t n, int kind, int fork, const lcv_update_batch* out,
                                      uint64_t* pool_src, uint64_t* npool_out, uint8_t* status) {
  if (!wire_fork_ok(fork)) return LCV_EINVAL;
  return decode_updates(buf, offsets, lengths, n, kind, [fork](uint64_t) { return fork; }, out, pool_src, npool_out,
                        status);
}

extern "C" int lcv_ssz_decode_updates_mixed(const uint8_t* buf, const uint64_t* offsets, const uint64_t* lengths,
                                            uint64_t n, int kind, const uint8_t* forks, const lcv_update_batch* out,
                                            uint64_t* pool_src, uint64_t* npool_out, uint8_t* status) {
  if (n && !forks) return LCV_EINVAL;
  return decode_updates(buf, offsets, lengths, n, kind, [forks](uint64_t i) { return (int)forks[i]; }, out, pool_src,
                        npool_out, status);
}

// The tuple a class of lcv_set_dedup is made of — attested beacon header, sync bits, signature, signature_slot — of
// every message, read where the messages lie (lcv_relay_async's grouping: no other column is stored); all zero for a
// malformed message, as its row is.  Not part of the ABI: the driver declares it (lcv_driver.inc)
namespace lcv {
void wire_dedup_tuples(const uint8_t* buf, const uint64_t* offsets, const uint64_t* lengths, uint64_t n, int kind, int fork,
                       const uint8_t* forks, uint8_t* beacon, uint8_t* bits, uint8_t* sig, uint64_t* slot) {
  parallel_rows(n, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; ++i) {
      Dest d = {};
      d.p[WC_ATT][WH_BEACON] = beacon + (uint64_t)K_BEACON * i;
      d.p[WC_BITS][0] = bits + (uint64_t)K_BITS * i;
      d.p[WC_SIG][0] = sig + (uint64_t)K_SIG * i;
      d.p[WC_SLOT][0] = reinterpret_cast<uint8_t*>(slot + i);
      uint64_t c;
      decode_msg(buf + offsets[i], lengths[i], (uint32_t)kind, forks ? (uint32_t)forks[i] : (uint32_t)fork, d, &c);
    }
  });
}
}  // namespace lcv

// LightClientBootstrap (sync-protocol.md:109-115; the layout's kind WIRE_BOOTSTRAP): input of
// initialize_light_client_store (:351-373)
extern "C" int lcv_ssz_decode_bootstrap(const uint8_t* buf, uint64_t len, int fork, uint8_t* beacon112,
                                        uint8_t* exec832, uint8_t* exec_branch128, uint8_t* committee24624,
                                        uint8_t* committee_branch160, uint8_t* status) {
  if (!buf || !beacon112 || !exec832 || !exec_branch128 || !committee24624 || !committee_branch160 || !status)
    return LCV_EINVAL;
  if (!wire_fork_ok(fork)) return LCV_EINVAL;
  Dest d = {};
  d.p[WC_ATT][WH_BEACON] = beacon112;
  d.p[WC_ATT][WH_EXEC] = exec832;
  d.p[WC_ATT][WH_BRANCH] = exec_branch128;
  d.p[WC_COMMITTEE][0] = committee24624;
  d.p[WC_NSC_BRANCH][0] = committee_branch160;
  uint64_t c;
  *status = decode_msg(buf, len, WIRE_BOOTSTRAP, (uint32_t)fork, d, &c) ? 0 : 1;
  return LCV_OK;
}
