// dedup_plan_check.cpp — stand-alone check of the host grouping behind lcv_set_dedup (csrc/lcv_dedup_plan.hpp), meant
// to be built with sanitizers: it calls dedup_classes and dedup_plan directly on random row patterns and compares
// them with a quadratic reference.  No device, no library.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I light-client-consensus-specs_amd/csrc tools/dedup_plan_check.cpp -o dedup_plan_check && ./dedup_plan_check
// Patterns: every row equal, every row distinct, few / many distinct updates, rows that differ in exactly one of the
// four key columns (first or last byte), one or many committee rows per class; hash widths 64, 7, 1 and 0 (every row
// collides: only the full compare separates rows); n from 1 to a few thousand, 0 included.
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "lcv_dedup_plan.hpp"

using namespace lcv;

struct Rows {
  std::vector<uint8_t> beacon, bits, sig;
  std::vector<uint64_t> slot;
  std::vector<uint32_t> comm;
};

static int failures = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      printf("FAILED %s (line %d, n %u, bits %u)\n", #x, __LINE__, n, hash_bits); \
      ++failures;                                                  \
      return;                                                      \
    }                                                              \
  } while (0)

static bool key_equal(const Rows& r, uint32_t a, uint32_t b) {
  return r.slot[a] == r.slot[b] && memcmp(&r.beacon[112 * (size_t)a], &r.beacon[112 * (size_t)b], 112) == 0 &&
         memcmp(&r.bits[64 * (size_t)a], &r.bits[64 * (size_t)b], 64) == 0 &&
         memcmp(&r.sig[96 * (size_t)a], &r.sig[96 * (size_t)b], 96) == 0;
}

static void check(const Rows& r, uint32_t n, uint32_t hash_bits, bool with_comm) {
  // exactly n entries each: the sanitizer sees any access past the rows
  std::vector<uint32_t> cls(n), rep(n), urow(n);
  DedupTable t;
  dedup_classes(r.beacon.data(), r.slot.data(), r.bits.data(), r.sig.data(), n, hash_bits, cls.data(), t);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t first = i;
    for (uint32_t a = 0; a < i; ++a)
      if (key_equal(r, a, i)) {
        first = a;
        break;
      }
    CHECK(cls[i] == first);
  }
  const uint32_t* comm = with_comm ? r.comm.data() : nullptr;
  const uint32_t m = dedup_plan(cls.data(), comm, n, hash_bits, rep.data(), urow.data(), t);
  CHECK(m <= n && (n == 0 || m >= 1));
  uint32_t seen = 0;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t first = i;
    for (uint32_t a = 0; a < i; ++a)
      if (cls[a] == cls[i] && (!comm || comm[a] == comm[i])) {
        first = a;
        break;
      }
    CHECK(rep[i] < m);
    if (first == i) {  // a new item: numbered by first appearance, its first row recorded
      CHECK(rep[i] == seen && urow[seen] == i);
      ++seen;
    } else {
      CHECK(rep[i] == rep[first]);
    }
  }
  CHECK(seen == m);
  for (uint32_t u = 1; u < m; ++u) CHECK(urow[u] > urow[u - 1]);
}

int main() {
  std::mt19937_64 rng(20240607);
  unsigned cases = 0;
  const uint32_t sizes[] = {0, 1, 2, 3, 63, 64, 65, 130, 1000, 4097};
  for (uint32_t n : sizes)
    for (int pattern = 0; pattern < 6; ++pattern) {
      // distinct updates the rows are drawn from: 1 (all equal), n (all distinct), 2, 7, n / 2, and a pool whose
      // members differ pairwise in one byte of one column only
      const uint32_t nd = pattern == 0 ? 1 : pattern == 1 ? (n ? n : 1) : pattern == 2 ? 2 : pattern == 3 ? 7
                        : pattern == 4 ? (n / 2 ? n / 2 : 1) : 9;
      Rows pool;
      pool.beacon.resize(112 * (size_t)nd); pool.bits.resize(64 * (size_t)nd); pool.sig.resize(96 * (size_t)nd);
      pool.slot.resize(nd);
      for (uint32_t d = 0; d < nd; ++d) {
        if (pattern == 5) {  // member 0 is all zero; member d > 0 differs from it in one place
          static const int where[8][2] = {{0, 0}, {0, 111}, {1, 0}, {1, 63}, {2, 0}, {2, 95}, {3, 0}, {3, 7}};
          const int* w = where[(d + 7) % 8];
          if (d == 0) continue;
          if (w[0] == 0) pool.beacon[112 * (size_t)d + w[1]] = 1;
          else if (w[0] == 1) pool.bits[64 * (size_t)d + w[1]] = 1;
          else if (w[0] == 2) pool.sig[96 * (size_t)d + w[1]] = 1;
          else pool.slot[d] = 1ull << (8 * w[1]);
          continue;
        }
        for (size_t k = 0; k < 112; ++k) pool.beacon[112 * (size_t)d + k] = (uint8_t)rng();
        for (size_t k = 0; k < 64; ++k) pool.bits[64 * (size_t)d + k] = (uint8_t)rng();
        for (size_t k = 0; k < 96; ++k) pool.sig[96 * (size_t)d + k] = (uint8_t)rng();
        pool.slot[d] = rng();
      }
      for (uint32_t stores = 1; stores <= 5; stores += 2) {
        Rows r;
        r.beacon.resize(112 * (size_t)n); r.bits.resize(64 * (size_t)n); r.sig.resize(96 * (size_t)n);
        r.slot.resize(n); r.comm.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
          const uint32_t d = pattern == 1 ? i : (uint32_t)(rng() % nd);
          memcpy(&r.beacon[112 * (size_t)i], &pool.beacon[112 * (size_t)d], 112);
          memcpy(&r.bits[64 * (size_t)i], &pool.bits[64 * (size_t)d], 64);
          memcpy(&r.sig[96 * (size_t)i], &pool.sig[96 * (size_t)d], 96);
          r.slot[i] = pool.slot[d];
          r.comm[i] = stores == 1 ? 0xFFFFFFFFu : (uint32_t)(rng() % stores) * 1000u;
        }
        const uint32_t widths[] = {64, 7, 1, 0};
        for (uint32_t hash_bits : widths) {
          if (hash_bits < 7 && n > 1000) continue;  // (every row on one probe chain: quadratic)
          check(r, n, hash_bits, false);
          check(r, n, hash_bits, true);
          cases += 2;
        }
      }
    }
  printf("dedup_plan_check: %u cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
