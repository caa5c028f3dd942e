// driver_alloc_check.cpp — stand-alone check of the driver's memory handling (csrc/lcv_driver.inc: DevBuf, PinBuf,
// Scratch, batch_new, the boundary `guarded`) on the host simulation, meant to be built with sanitizers.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -pthread -fopenmp -DLCV_ALLOC_CHECK -Wl,--wrap=_Znwm -Wl,--wrap=_Znam -I light-client-consensus-specs_amd/build \
//       tools/driver_alloc_check.cpp light-client-consensus-specs_amd/csrc/lcv_wire.cpp -o driver_alloc_check
// It includes the host simulation, whose LCV_ALLOC_CHECK hook counts the live device and pinned allocations and fails
// the k-th allocation on request.
// (a) For every scenario below, and k = 0, 1, 2, ... until the call makes fewer than k + 1 device or pinned
//     allocations: on a fresh context, with allocation k of the call failing, the call returns LCV_ENOMEM with a
//     message; the same call again, with nothing failing, succeeds; and its outputs equal those of a fresh context on
//     which nothing ever failed.  The batches have at most 2 all-zero rows: the allocation paths do not depend on
//     what the rows hold.
// (b) With a replacement operator new that throws std::bad_alloc on its n-th call on this thread: every host
//     allocation that lcv_set_store_table and lcv_fast_aggregate_verify (3 keys) make ahead of their first device
//     allocation fails once; each call returns LCV_ENOMEM, and no exception leaves the library.
// (c) After lcv_destroy no device or pinned allocation is live (and LeakSanitizer reports nothing at exit).
// Prints its counts; exit status 1 on any failure.  No device, no library, nothing loaded into an interpreter.
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
};

static int validate_resident_2(lcv_ctx* c, Bytes& o) {
  ZeroBatch zb(2);
  lcv_dbatch* db = nullptr;
  LCV_TRY(lcv_batch_upload(c, &zb.hb, &db));
  uint8_t out[4] = {0xEE, 0xEE, 0xEE, 0xEE};
  const int rc = lcv_validate_resident(c, db, kNow, kGvr, out, out + 2);
  lcv_batch_free(c, db);
  if (rc == LCV_OK) put(o, out, 4);
  return rc;
}

static std::vector<Scenario> scenarios() {
  std::vector<Scenario> v;
  auto nothing = [](lcv_ctx*) { return (int)LCV_OK; };
  v.push_back({"lcv_set_store", nothing, [](lcv_ctx* c, Bytes& o) {
    uint8_t status[1024];
    LCV_TRY(lcv_set_store(c, 0, kZero.data(), kZero.data(), status));
    put(o, status, 1024);
    return (int)LCV_OK;
  }});
  v.push_back({"lcv_set_store_table", nothing, [](lcv_ctx* c, Bytes& o) { return set_table(c, &o); }});
  v.push_back({"lcv_validate_updates", set_store, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(1);
    uint8_t out[2] = {0xEE, 0xEE};
    LCV_TRY(lcv_validate_updates(c, &zb.hb, kNow, kGvr, out, out + 1));
    put(o, out, 2);
    return (int)LCV_OK;
  }});
  v.push_back({"lcv_validate_async + lcv_slot_wait", set_store, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(2);
    uint8_t out[4] = {0xEE, 0xEE, 0xEE, 0xEE};
    LCV_TRY(lcv_validate_async(c, &zb.hb, kNow, kGvr, 1));
    LCV_TRY(lcv_slot_wait(c, 1, 2, out, out + 2));
    put(o, out, 4);
    return (int)LCV_OK;
  }});
  v.push_back({"lcv_validate_stores_fold", [](lcv_ctx* c) { return set_table(c); }, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(2);
    const uint32_t six[2] = {1, 0};
    lcv_fold_state in[2];
    lcv_fold_result res[2];
    memset(in, 0, sizeof in);
    memset(res, 0xEE, sizeof res);
    uint8_t out[4] = {0xEE, 0xEE, 0xEE, 0xEE};
    LCV_TRY(lcv_validate_stores_fold(c, &zb.hb, six, kNow, kGvr, in, out, out + 2, res));
    put(o, out, 4);
    put(o, res, 2);
    return (int)LCV_OK;
  }});
  v.push_back({"resident batch under lcv_set_dedup",
               [](lcv_ctx* c) { LCV_TRY(set_store(c)); LCV_TRY(lcv_set_latency_mode(c, 0)); return lcv_set_dedup(c, 1); },
               [](lcv_ctx* c, Bytes& o) {
    LCV_TRY(validate_resident_2(c, o));
    uint64_t rows = 0, items = 0;
    LCV_TRY(lcv_last_dedup(c, 0, &rows, &items));
    put(o, &rows, 1);
    put(o, &items, 1);
    return (int)LCV_OK;
  }});
  v.push_back({"resident batch under lcv_set_rlc, latency mode off", [](lcv_ctx* c) {
    uint8_t seed[32];
    memset(seed, 7, 32);
    LCV_TRY(set_store(c));
    LCV_TRY(lcv_set_latency_mode(c, 0));
    return lcv_set_rlc(c, 2, seed);
  }, [](lcv_ctx* c, Bytes& o) {
    LCV_TRY(validate_resident_2(c, o));
    uint64_t groups = 0, retried = 0;
    LCV_TRY(lcv_last_rlc(c, 0, &groups, &retried));
    put(o, &groups, 1);
    put(o, &retried, 1);
    return (int)LCV_OK;
  }});
  v.push_back({"lcv_batch_upload", nothing, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(2);
    lcv_dbatch* db = nullptr;
    LCV_TRY(lcv_batch_upload(c, &zb.hb, &db));
    uint64_t shape[2] = {0, 0};
    const int rc = lcv_batch_shape(c, db, &shape[0], &shape[1]);
    lcv_batch_free(c, db);
    put(o, shape, 2);
    return rc;
  }});
  v.push_back({"lcv_create_updates_resident + lcv_batch_download (row list)", nothing, [](lcv_ctx* c, Bytes& o) {
    ZeroViews zv;
    const uint32_t ix[2] = {0, 0};
    const int32_t fin[2] = {-1, 0};
    const lcv_update_cases cases = {ix, ix, ix, ix, fin};
    uint8_t reason[2] = {0xEE, 0xEE};
    lcv_dbatch* db = nullptr;
    LCV_TRY(lcv_create_updates_resident(c, &zv.s, 1, &zv.b, 1, kZero.data(), 1, &cases, 2, 0, reason, &db));
    const uint32_t rows[3] = {1, 0, 1};
    OutBatch ob(3, 2);
    const int rc = lcv_batch_download(c, db, rows, 3, &ob.hb);
    lcv_batch_free(c, db);
    put(o, reason, 2);
    ob.append_to(o);
    return rc;
  }});
  v.push_back({"lcv_rank_updates", nothing, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(2);
    uint8_t rank[2 * LCV_RANK_BYTES];
    memset(rank, 0xEE, sizeof rank);
    LCV_TRY(lcv_rank_updates(c, &zb.hb, rank));
    put(o, rank, sizeof rank);
    return (int)LCV_OK;
  }});
  v.push_back({"lcv_batch_encode", nothing, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(2);
    lcv_dbatch* db = nullptr;
    LCV_TRY(lcv_batch_upload(c, &zb.hb, &db));
    Bytes out(2 * lcv_encode_pitch(1), 0xEE);
    uint32_t len[2] = {0, 0};
    uint8_t meta[2 + 8 + 2];
    memset(meta, 0xEE, sizeof meta);
    const int rc = lcv_batch_encode(c, db, nullptr, 0, 1, 0, out.data(), len, meta, meta + 2, meta + 10);
    lcv_batch_free(c, db);
    if (rc == LCV_OK) {
      for (int i = 0; i < 2; ++i) put(o, out.data() + i * lcv_encode_pitch(1), len[i]);
      put(o, len, 2);
      put(o, meta, sizeof meta);
    }
    return rc;
  }});
  for (int kind = 1; kind >= 0; --kind)
    v.push_back({kind ? "lcv_batch_decode, kind 1" : "lcv_batch_decode, kind 0", nothing, [kind](lcv_ctx* c, Bytes& o) {
      // Altair-format messages (fixed size), all zero
      const uint64_t len = kind ? 112 + 112 + 192 + 168 : 112 + 24624 + 160 + 112 + 192 + 168;
      const uint64_t offs[2] = {0, 16}, lens[2] = {len, len};
      uint8_t status[2] = {0xEE, 0xEE};
      lcv_dbatch* db = nullptr;
      LCV_TRY(lcv_batch_decode(c, kZero.data(), kZero.size(), offs, lens, 2, kind, 2, nullptr, status, &db));
      uint64_t shape[2] = {0, 0};
      lcv_batch_shape(c, db, &shape[0], &shape[1]);
      OutBatch ob(shape[0], shape[1]);
      const int rc = lcv_batch_download(c, db, nullptr, 0, &ob.hb);
      lcv_batch_free(c, db);
      put(o, shape, 2);
      put(o, status, 2);
      ob.append_to(o);
      return rc;
    }});
  v.push_back({"lcv_fast_aggregate_verify, 45-byte message", nothing, [](lcv_ctx* c, Bytes& o) {
    int result = -1;
    LCV_TRY(lcv_fast_aggregate_verify(c, kZero.data(), 3, kZero.data(), 45, kZero.data(), &result));
    put(o, &result, 1);
    return (int)LCV_OK;
  }});
  v.push_back({"lcv_htr_sync_committee_batch (simple_call)", nothing, [](lcv_ctx* c, Bytes& o) {
    uint8_t roots[64];
    memset(roots, 0xEE, sizeof roots);
    LCV_TRY(lcv_htr_sync_committee_batch(c, kZero.data(), 2, roots));
    put(o, roots, 64);
    return (int)LCV_OK;
  }});
  v.push_back({"lcv_debug_fold", nothing, [](lcv_ctx* c, Bytes& o) {
    lcv_fold_state in;
    lcv_fold_result res;
    memset(&in, 0, sizeof in);
    memset(&res, 0xEE, sizeof res);
    LCV_TRY(lcv_debug_fold(c, kZero.data(), kZero.data(), 2, 0, 1, &in, &res));
    put(o, &res, 1);
    return (int)LCV_OK;
  }});
  v.push_back({"lcv_debug_fold_stores", nothing, [](lcv_ctx* c, Bytes& o) {
    const uint32_t six[2] = {1, 0};
    const uint64_t fin[2] = {0, 0};
    const uint8_t known[2] = {1, 0};
    lcv_fold_state in[2];
    lcv_fold_result res[2];
    memset(in, 0, sizeof in);
    memset(res, 0xEE, sizeof res);
    LCV_TRY(lcv_debug_fold_stores(c, kZero.data(), kZero.data(), six, 2, fin, known, 2, in, res));
    put(o, res, 2);
    return (int)LCV_OK;
  }});
  return v;
}

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

// (a)
static void sweep(const Scenario& s) {
  Bytes want;
  lcv_ctx* c = fresh(s);
  const long a0 = g_allocs;
  const int rc0 = s.call(c, want);
  const long made = g_allocs - a0;
  CHECK(rc0 == LCV_OK, "%s: %d on a fresh context (%s)", s.name, rc0, lcv_last_error(c));
  destroy(c, s.name);
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
      const int rc2 = s.call(c, got);
      CHECK(rc2 == LCV_OK, "%s: after allocation %ld failed, the same call returned %d (%s)", s.name, k, rc2, lcv_last_error(c));
      CHECK(got == want, "%s: after allocation %ld failed, the same call's outputs differ from a fresh context's", s.name, k);
    } else {
      CHECK(rc == LCV_OK && k == made, "%s: %ld allocations on a fresh context, %ld in the sweep (rc %d)", s.name, made, k, rc);
    }
    destroy(c, s.name);
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
    destroy(c, s.name);
    if (!injected || escaped) break;
  }
  CHECK(n >= expect_at_least, "%s: %ld host allocations ahead of the first device allocation, expected %ld", s.name, n, expect_at_least);
}

int main() {
  const std::vector<Scenario> all = scenarios();
  for (const Scenario& s : all) sweep(s);
  for (const Scenario& s : all) {
    if (!strcmp(s.name, "lcv_set_store_table")) host_sweep(s, 4);  // zero_row, next, and the two host columns
    if (!strncmp(s.name, "lcv_fast_aggregate_verify", 25)) host_sweep(s, 3);  // table, bits, cid
  }
  printf("driver_alloc_check: %llu scenarios, %llu device or pinned injections, %llu host injections, %llu failures\n",
         n_scenarios, n_injections, n_host_injections, failures);
  return failures ? 1 : 0;
}
