// lcv_dedup_plan.hpp — host side of the deduplicated BLS half (lcv_set_dedup, include/lcv.h "Deduplicated
// signatures"): rows whose BLS inputs are bytewise equal are grouped, so the device checks each distinct signature
// once.  Plain C++ over the standard library only: the driver (lcv_driver.inc) and the stand-alone sanitizer check
// (tools/dedup_plan_check.cpp) both include it.
//   dedup_classes  store-independent class of every row: rows with equal (attested beacon header, signature_slot,
//                  sync_committee_bits, sync_committee_signature) get the index of the first such row
//   dedup_plan     the grouping of one chunk: rows with equal (class, committee row) are one item
//   dedup_confirm_groups  the host loop of a grouping whose full compares run elsewhere (on the device, on threads)
//   dedup_pool_rows       the numbering of a decoded batch's committee pool (the host and the device wire decoders)
// Both are one pass over an open-addressing table: O(n) expected.  Rows are merged only on a full compare of their
// keys; the hash only picks where to look (hash_bits < 64 truncates it — 0 makes every row collide — so tests can
// show that).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace lcv {

enum { DEDUP_BEACON = 112, DEDUP_BITS = 64, DEDUP_SIG = 96 };

// scratch of the grouping passes, kept by the caller so that a serving loop allocates once
struct DedupTable {
  std::vector<uint32_t> row;   // row + 1 of the entry's first row, 0 = empty
  std::vector<uint64_t> hash;  // the entry's (truncated) hash
};

inline uint64_t dedup_mix(uint64_t h, uint64_t x) {
  h = (h ^ x) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
inline uint64_t dedup_hash_bytes(uint64_t h, const uint8_t* p, size_t bytes) {  // bytes % 8 == 0
  for (size_t k = 0; k < bytes; k += 8) {
    uint64_t x;
    memcpy(&x, p + k, 8);
    h = dedup_mix(h, x);
  }
  return h;
}
inline uint64_t dedup_truncate(uint64_t h, uint32_t hash_bits) {
  return hash_bits >= 64 ? h : hash_bits == 0 ? 0 : h & ((1ull << hash_bits) - 1);
}

// One grouping pass over rows 0 .. n-1 in order: hash(i) picks the probe start, equal(a, i) is the full compare of
// row i with the earlier row a, first(i) is called for a row that equals no earlier one and same(a, i) for one that
// equals row a, the first of its group.
template <class Hash, class Equal, class First, class Same>
inline void dedup_group(uint32_t n, uint32_t hash_bits, DedupTable& t, Hash hash, Equal equal, First first, Same same) {
  size_t cap = 16;
  while (cap < 2 * (size_t)n) cap *= 2;
  t.row.assign(cap, 0u);
  t.hash.resize(cap);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t h = dedup_truncate(hash(i), hash_bits);
    for (size_t j = (size_t)dedup_mix(0, h) & (cap - 1);; j = (j + 1) & (cap - 1)) {
      const uint32_t e = t.row[j];
      if (e == 0) {
        t.row[j] = i + 1;
        t.hash[j] = h;
        first(i);
        break;
      }
      if (t.hash[j] == h && equal(e - 1, i)) {
        same(e - 1, i);
        break;
      }
    }
  }
}

// cls[i] = the first row whose (attested beacon, signature_slot, bits, signature) equal row i's
inline void dedup_classes(const uint8_t* att_beacon, const uint64_t* sig_slot, const uint8_t* bits, const uint8_t* sig,
                          uint32_t n, uint32_t hash_bits, uint32_t* cls, DedupTable& t) {
  dedup_group(
      n, hash_bits, t,
      [&](uint32_t i) {
        uint64_t h = dedup_mix(0x6c63765f64656475ull, sig_slot[i]);
        h = dedup_hash_bytes(h, sig + (size_t)DEDUP_SIG * i, DEDUP_SIG);
        h = dedup_hash_bytes(h, att_beacon + (size_t)DEDUP_BEACON * i, DEDUP_BEACON);
        return dedup_hash_bytes(h, bits + (size_t)DEDUP_BITS * i, DEDUP_BITS);
      },
      [&](uint32_t a, uint32_t i) {
        return sig_slot[a] == sig_slot[i] &&
               memcmp(sig + (size_t)DEDUP_SIG * a, sig + (size_t)DEDUP_SIG * i, DEDUP_SIG) == 0 &&
               memcmp(att_beacon + (size_t)DEDUP_BEACON * a, att_beacon + (size_t)DEDUP_BEACON * i, DEDUP_BEACON) == 0 &&
               memcmp(bits + (size_t)DEDUP_BITS * a, bits + (size_t)DEDUP_BITS * i, DEDUP_BITS) == 0;
      },
      [&](uint32_t i) { cls[i] = i; }, [&](uint32_t a, uint32_t i) { cls[i] = a; });
}

// Groups made on a hash alone, settled by full compares somebody else runs (the device: lcv_batch_decode's committee
// pool, lcv_batch_classify's classes).  rep[r] = the tentative representative of row r, the first row of its hash
// group (rep[r] == r for a representative; rows outside the grouping are never looked at); `pending` lists, ascending,
// the rows with rep[r] != r.  confirm(pending, rep, differ) compares row pending[k] with row rep[pending[k]] in full
// for every k, sets differ[k] (pending.size() entries, non-zero: they differ) and returns 0, or an error code, which
// ends the loop.  The rows of a group that differ form the next candidate group under their lowest row, which becomes
// a representative, and the compare repeats: one call per extra distinct content under one hash value.  On return
// rep[r] is the first row whose content equals row r's.
template <class Confirm>
inline int dedup_confirm_groups(std::vector<uint32_t>& rep, std::vector<uint32_t>& pending, Confirm confirm) {
  const uint32_t none = 0xffffffffu;
  std::vector<uint32_t> next, differ, touched, newrep(rep.size(), none);
  while (!pending.empty()) {
    const size_t m = pending.size();
    differ.assign(m, 0u);
    const int rc = confirm(pending, rep, differ);
    if (rc != 0) return rc;
    next.clear();
    touched.clear();
    for (size_t k = 0; k < m; ++k) {
      if (!differ[k]) continue;
      const uint32_t r = pending[k], old = rep[r];
      if (newrep[old] == none) {  // the lowest differing row of its group: a representative of its own
        newrep[old] = r;
        touched.push_back(old);
        rep[r] = r;
      } else {
        rep[r] = newrep[old];
        next.push_back(r);
      }
    }
    for (uint32_t old : touched) newrep[old] = none;
    pending.swap(next);
  }
  return 0;
}

// The committee pool of a decoded batch (lcv_ssz_decode_updates, lcv_batch_decode) from its grouping: rep[i] = the
// first row whose committee equals row i's, or 0xffffffff for a row without one, which stands for SyncCommittee().
// Pool rows are numbered in order of first occurrence and SyncCommittee() takes a row at its first use: index[i] =
// row i's pool row, first[k] = the first row of pool row k, or 0xffffffff for the row of SyncCommittee().
inline void dedup_pool_rows(const std::vector<uint32_t>& rep, uint32_t* index, std::vector<uint32_t>& first) {
  const uint32_t none = 0xffffffffu;
  uint32_t zero_ix = none;
  first.clear();
  for (uint32_t i = 0; i < (uint32_t)rep.size(); ++i) {
    if (rep[i] == none) {
      if (zero_ix == none) {
        zero_ix = (uint32_t)first.size();
        first.push_back(none);
      }
      index[i] = zero_ix;
    } else if (rep[i] == i) {
      index[i] = (uint32_t)first.size();
      first.push_back(i);
    } else {
      index[i] = index[rep[i]];  // (rep[i] < i)
    }
  }
}

// The grouping of a chunk of n rows: row i has class cls[i] (any labels: equal labels = equal BLS inputs apart from
// the committee) and is checked against committee row comm[i] (comm null: one committee choice per class, the
// single-store case).  rep[i] = the item of row i, urow[u] = the first row of item u — ascending, so the numbering
// is that of first appearance — and the number of items is returned.  rep and urow hold n entries each.
inline uint32_t dedup_plan(const uint32_t* cls, const uint32_t* comm, uint32_t n, uint32_t hash_bits, uint32_t* rep,
                           uint32_t* urow, DedupTable& t) {
  uint32_t m = 0;
  dedup_group(
      n, hash_bits, t, [&](uint32_t i) { return dedup_mix(dedup_mix(0, cls[i]), comm ? comm[i] : 0u); },
      [&](uint32_t a, uint32_t i) { return cls[a] == cls[i] && (!comm || comm[a] == comm[i]); },
      [&](uint32_t i) {
        urow[m] = i;
        rep[i] = m++;
      },
      [&](uint32_t a, uint32_t i) { rep[i] = rep[a]; });
  return m;
}

}  // namespace lcv
