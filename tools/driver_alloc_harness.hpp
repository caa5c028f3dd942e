// driver_alloc_harness.hpp — what the stand-alone allocation checks of the driver share (tools/driver_alloc_check.cpp,
// tools/dedup_class_check.cpp): the host simulation with its LCV_ALLOC_CHECK hook (the live device and pinned
// allocations are counted and the k-th one fails on request), a replacement operator new that throws on its n-th call,
// all-zero inputs, and the two sweeps.
//   sweep       (a) for k = 0, 1, 2, ... until the call makes fewer than k + 1 device or pinned allocations: on a fresh
//               context, with allocation k of the call failing, the call returns LCV_ENOMEM with a message; the same call
//               again, with nothing failing, succeeds; and its outputs equal those of a fresh context on which nothing
//               ever failed.  A scenario may look at the context between the failure and the retry (after_failure)
//   host_sweep  (b) every host allocation the call makes ahead of its first device allocation fails once: the call
//               returns LCV_ENOMEM, and no exception leaves the library
//   destroy     (c) after lcv_destroy no device or pinned allocation is live
// Build flags: see either program.
#pragma once
#include <stdio.h>

#include <functional>

#include "../light-client-consensus-specs_amd/csrc/lcv_hostsim.cpp"

typedef std::vector<uint8_t> Bytes;

// ---- (b) the replacement operator new: the n-th call on the arming thread throws, while no backend allocation has
// been made since it was armed.  The sanitizer's static runtime defines operator new itself, so the replacement is
// linked in front of it (-Wl,--wrap): every call of operator new from this program's code comes here first
static thread_local long t_new_fail_in = -1;
static thread_local long t_new_allocs0 = 0;
static void maybe_throw() {
  if (t_new_fail_in >= 0 && g_allocs == t_new_allocs0 && t_new_fail_in-- == 0) throw std::bad_alloc();
}
extern "C" {
void* __real__Znwm(size_t n);
void* __real__Znam(size_t n);
void* __wrap__Znwm(size_t n) { maybe_throw(); return __real__Znwm(n); }  // operator new(size_t)
void* __wrap__Znam(size_t n) { maybe_throw(); return __real__Znam(n); }  // operator new[](size_t)
}

static unsigned long long n_scenarios = 0, n_injections = 0, n_host_injections = 0, failures = 0;
#define CHECK(x, ...)                                                      \
  do {                                                                     \
    if (!(x)) {                                                            \
      printf("FAILED %s (line %d): ", #x, __LINE__);                       \
      printf(__VA_ARGS__);                                                 \
      printf("\n");                                                        \
      if (++failures > 20) exit(1);                                        \
    }                                                                      \
  } while (0)

// ---- inputs: all-zero columns
struct ZeroBatch {
  Bytes mem;
  std::vector<uint32_t> index;
  std::vector<uint64_t> slot;
  lcv_update_batch hb;
  explicit ZeroBatch(size_t n) : mem(LCV_SYNC_COMMITTEE_BYTES + 1024 * n, 0), index(n, 0), slot(n, 0) {
    const uint8_t* z = mem.data();
    hb.attested = hb.finalized = lcv_header_cols{z, z, z};
    hb.nsc_pool = z;
    hb.nsc_index = index.data();
    hb.nsc_branch = hb.finality_branch = hb.sync_bits = hb.sync_signature = z;
    hb.signature_slot = slot.data();
    hb.n = n;
    hb.npool = 1;
  }
};
// writable columns of n rows and a pool of npool rows (lcv_batch_download)
struct OutBatch {
  Bytes col[10], pool;
  std::vector<uint32_t> index;
  std::vector<uint64_t> slot;
  lcv_update_batch hb;
  OutBatch(size_t n, size_t npool) : pool(LCV_SYNC_COMMITTEE_BYTES * npool, 0xEE), index(n, 0xEEEEEEEEu), slot(n, 0) {
    const size_t w[10] = {112, 832, 128, 112, 832, 128, 160, 192, 64, 96};
    for (int k = 0; k < 10; ++k) col[k].assign(w[k] * n, 0xEE);
    hb.attested = lcv_header_cols{col[0].data(), col[1].data(), col[2].data()};
    hb.finalized = lcv_header_cols{col[3].data(), col[4].data(), col[5].data()};
    hb.nsc_pool = pool.data();
    hb.nsc_index = index.data();
    hb.nsc_branch = col[6].data(); hb.finality_branch = col[7].data(); hb.sync_bits = col[8].data();
    hb.sync_signature = col[9].data();
    hb.signature_slot = slot.data();
    hb.n = n;
    hb.npool = npool;
  }
  void append_to(Bytes& o) const {
    for (int k = 0; k < 10; ++k) o.insert(o.end(), col[k].begin(), col[k].end());
    o.insert(o.end(), pool.begin(), pool.end());
    o.insert(o.end(), (const uint8_t*)index.data(), (const uint8_t*)(index.data() + index.size()));
    o.insert(o.end(), (const uint8_t*)slot.data(), (const uint8_t*)(slot.data() + slot.size()));
  }
};
template <class T> static void put(Bytes& o, const T* p, size_t n) { o.insert(o.end(), (const uint8_t*)p, (const uint8_t*)(p + n)); }

static const Bytes kZero(2 * LCV_SYNC_COMMITTEE_BYTES + 4096, 0);
static const uint8_t kGvr[32] = {};
static const uint64_t kNow = 1000;

static int set_store(lcv_ctx* c) { return lcv_set_store(c, 0, kZero.data(), kZero.data(), nullptr); }
static int set_table(lcv_ctx* c, Bytes* o = nullptr) {
  const uint64_t fin[2] = {0, 0};
  const uint32_t cur[2] = {0, 1}, next[2] = {1, LCV_STORE_NEXT_UNKNOWN};
  const lcv_store_table t = {kZero.data(), 2, fin, cur, next, 2};
  uint8_t status[1024];
  memset(status, 0xEE, sizeof status);
  const int rc = lcv_set_store_table(c, &t, status);
  if (o && rc == LCV_OK) put(*o, status, 1024);
  return rc;
}
// the producer's views: one state, one block, one committee, all zero
struct ZeroViews {
  Bytes z;
  uint32_t ix[2] = {0, 0};
  uint64_t u[2] = {0, 0};
  lcv_state_views s;
  lcv_block_views b;
  ZeroViews() : z(32 * 28 + 1024, 0) {
    s = lcv_state_views{u, z.data(), u, z.data(), z.data(), ix, ix};
    b = lcv_block_views{u, u, z.data(), z.data(), z.data(), z.data(), z.data(), z.data(), z.data()};
  }
};

// A scenario: `prepare` (never failing) brings a fresh context to the state the call needs; `call` is what the sweep
// fails and repeats, appending its outputs
struct Scenario {
  const char* name;
  std::function<int(lcv_ctx*)> prepare;
  std::function<int(lcv_ctx*, Bytes&)> call;
  std::function<void(lcv_ctx*)> release;  // (optional) frees what `prepare` left for `call`, ahead of lcv_destroy
  // (optional) runs after each injected failure and before the retry: what the failed call left behind must be usable
  std::function<void(lcv_ctx*, const char* name, long k)> after_failure;
  long min_allocs = 0;  // the call must make at least this many allocations for the scenario to test what it is meant to
};


static lcv_ctx* fresh(const Scenario& s) {
  lcv_ctx* c = nullptr;
  if (lcv_init(0, &c) != LCV_OK || s.prepare(c) != LCV_OK) {
    printf("FAILED: %s: no context (%s)\n", s.name, lcv_last_error(c));
    exit(1);
  }
  return c;
}
// (c)
static void destroy(lcv_ctx* c, const char* what) {
  lcv_destroy(c);
  CHECK(g_live[0] == 0 && g_live[1] == 0, "%s: %ld device and %ld pinned allocations live after lcv_destroy", what, g_live[0], g_live[1]);
  g_live[0] = g_live[1] = 0;
}

static void finish(const Scenario& s, lcv_ctx* c) {
  if (s.release) s.release(c);
  destroy(c, s.name);
}

// (a)
static void sweep(const Scenario& s) {
  Bytes want;
  lcv_ctx* c = fresh(s);
  const long a0 = g_allocs;
  const int rc0 = s.call(c, want);
  const long made = g_allocs - a0;
  CHECK(rc0 == LCV_OK, "%s: %d on a fresh context (%s)", s.name, rc0, lcv_last_error(c));
  CHECK(made >= s.min_allocs, "%s: %ld allocations, the scenario needs %ld", s.name, made, s.min_allocs);
  finish(s, c);
  ++n_scenarios;
  for (long k = 0;; ++k) {
    c = fresh(s);
    Bytes got, junk;
    g_fail_in = k;
    const int rc = s.call(c, junk);
    const bool injected = g_fail_in < 0;
    g_fail_in = -1;
    if (injected) {
      ++n_injections;
      CHECK(rc == LCV_ENOMEM, "%s: allocation %ld failing: returned %d", s.name, k, rc);
      CHECK(lcv_last_error(c)[0] != 0, "%s: allocation %ld failing: no message", s.name, k);
      if (s.after_failure) s.after_failure(c, s.name, k);
      const int rc2 = s.call(c, got);
      CHECK(rc2 == LCV_OK, "%s: after allocation %ld failed, the same call returned %d (%s)", s.name, k, rc2, lcv_last_error(c));
      CHECK(got == want, "%s: after allocation %ld failed, the same call's outputs differ from a fresh context's", s.name, k);
    } else {
      CHECK(rc == LCV_OK && k == made, "%s: %ld allocations on a fresh context, %ld in the sweep (rc %d)", s.name, made, k, rc);
    }
    finish(s, c);
    if (!injected) break;
  }
  printf("%-60s %ld allocations\n", s.name, made);
  fflush(stdout);
}

// (b)
static void host_sweep(const Scenario& s, long expect_at_least) {
  long n = 0;
  for (;; ++n) {
    lcv_ctx* c = fresh(s);
    Bytes junk, got;
    int rc = LCV_OK;
    bool escaped = false;
    t_new_allocs0 = g_allocs;
    t_new_fail_in = n;
    try {
      rc = s.call(c, junk);
    } catch (...) {
      escaped = true;
    }
    const bool injected = t_new_fail_in < 0;
    t_new_fail_in = -1;
    CHECK(!escaped, "%s: host allocation %ld failing: an exception left the library", s.name, n);
    if (injected) {
      ++n_host_injections;
      CHECK(rc == LCV_ENOMEM, "%s: host allocation %ld failing: returned %d", s.name, n, rc);
      const int rc2 = s.call(c, got);
      CHECK(rc2 == LCV_OK, "%s: after host allocation %ld failed, the same call returned %d (%s)", s.name, n, rc2, lcv_last_error(c));
    }
    finish(s, c);
    if (!injected || escaped) break;
  }
  CHECK(n >= expect_at_least, "%s: %ld host allocations ahead of the first device allocation, expected %ld", s.name, n, expect_at_least);
}
