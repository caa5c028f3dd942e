// dedup_class_check.cpp — stand-alone memory-safety and equivalence check of the classes of a resident batch
// (csrc/lcv_dedup.hpp: F_dedup_key, F_dedup_confirm; csrc/lcv_driver.inc: lcv_batch_classify, lcv_batch_fan_out) on the
// host simulation, meant to be built with sanitizers.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -pthread -fopenmp -DLCV_ALLOC_CHECK -Wl,--wrap=_Znwm -Wl,--wrap=_Znam -I light-client-consensus-specs_amd/build \
//       tools/dedup_class_check.cpp light-client-consensus-specs_amd/csrc/lcv_wire.cpp -o dedup_class_check
// (a) The two functors' rounds run lane by lane over heap buffers of EXACTLY the column, key, pair and flag sizes, the
//     LDS area pre-filled with garbage: an access one byte out of any of them is a sanitizer report.  Between them the
//     host's part runs as lcv_batch_classify runs it (dedup_group over the keys alone, dedup_confirm_groups), and the
//     class column is compared with dedup_classes over the same columns.  Batches: seeded ones of 1 .. 200 rows with
//     random duplication (whole rows, and rows differing from another in one tuple byte), and the 281-row table — row 0,
//     then row 0 with one bit flipped at each of the 280 tuple byte positions; hash widths 64, 7, 1 and 0.
// (b) Every device, pinned and early host allocation of lcv_batch_classify and lcv_batch_fan_out fails once
//     (tools/driver_alloc_harness.hpp: sweep, host_sweep), and nothing is live after lcv_destroy.
// Prints its counts; exit status 1 on any failure.  No device, no library, nothing loaded into an interpreter.
#include <memory>
#include <random>

#include "driver_alloc_harness.hpp"

static std::mt19937_64 rng(0x636c6173u);
static uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }

// ---- (a) a batch's four tuple columns, each an allocation of exactly its size
struct Columns {
  uint32_t n;
  std::unique_ptr<uint8_t[]> beacon, bits, sig;
  std::unique_ptr<uint64_t[]> slot;
  explicit Columns(uint32_t rows)
      : n(rows), beacon(new uint8_t[112 * (size_t)rows]), bits(new uint8_t[64 * (size_t)rows]),
        sig(new uint8_t[96 * (size_t)rows]), slot(new uint64_t[rows]) {}
  uint8_t* byte(uint32_t row, uint32_t k) {  // tuple byte k of a row: beacon, bits, signature, signature_slot
    if (k < 112) return &beacon[112 * (size_t)row + k];
    if (k < 176) return &bits[64 * (size_t)row + k - 112];
    if (k < 272) return &sig[96 * (size_t)row + k - 176];
    return (uint8_t*)&slot[row] + (k - 272);
  }
  void random_row(uint32_t row) {
    for (uint32_t k = 0; k < 280; ++k) *byte(row, k) = (uint8_t)rng();
  }
  void copy_row(uint32_t dst, uint32_t src) {
    for (uint32_t k = 0; k < 280; ++k) *byte(dst, k) = *byte(src, k);
  }
  BatchDev view() const {
    BatchDev B = BatchDev();
    B.att_beacon = beacon.get();
    B.bits = bits.get();
    B.sig = sig.get();
    B.sig_slot = slot.get();
    B.n = n;
    return B;
  }
};

// one team kernel, lane by lane, every item on a fresh LDS area of exactly F::LDS_WORDS words of garbage
template <class F> static void run_team(const F& f, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    std::unique_ptr<uint32_t[]> lds(new uint32_t[F::LDS_WORDS]);
    for (uint32_t k = 0; k < F::LDS_WORDS; ++k) lds[k] = 0xA5A5A5A5u ^ (uint32_t)rng();
    const uint32_t R = f.rounds();
    for (uint32_t r = 0; r < R; ++r)
      for (uint32_t lane = 0; lane < F::TEAM; ++lane) f(i, lane, r, lds.get(), nullptr);
  }
}

static unsigned long long n_batches = 0, n_rows = 0, n_confirm_launches = 0, n_pairs = 0;

// lcv_batch_classify's steps over `c` under a hash of hash_bits bits, against dedup_classes
static void classify_check(Columns& c, uint32_t hash_bits, const char* what) {
  const uint32_t n = c.n;
  const BatchDev B = c.view();
  std::unique_ptr<uint64_t[]> key(new uint64_t[n]);
  run_team(F_dedup_key{B, key.get()}, n);
  std::vector<uint32_t> cls(n), pending, want(n);
  DedupTable t;
  dedup_group(
      n, hash_bits, t, [&](uint32_t i) { return key[i]; }, [](uint32_t, uint32_t) { return true; },
      [&](uint32_t i) { cls[i] = i; }, [&](uint32_t a, uint32_t i) { cls[i] = a; });
  for (uint32_t i = 0; i < n; ++i)
    if (cls[i] != i) pending.push_back(i);
  dedup_confirm_groups(cls, pending, [&](const std::vector<uint32_t>& pend, const std::vector<uint32_t>& rp,
                                         std::vector<uint32_t>& differ) -> int {
    const uint32_t m = (uint32_t)pend.size();
    std::unique_ptr<uint32_t[]> pairs(new uint32_t[2 * (size_t)m]), flags(new uint32_t[m]);
    for (uint32_t k = 0; k < m; ++k) {
      pairs[2 * k] = pend[k];
      pairs[2 * k + 1] = rp[pend[k]];
      flags[k] = 0xEEEEEEEEu;
    }
    run_team(F_dedup_confirm{B, pairs.get(), flags.get()}, m);
    for (uint32_t k = 0; k < m; ++k) differ[k] = flags[k];
    ++n_confirm_launches;
    n_pairs += m;
    return 0;
  });
  dedup_classes(c.beacon.get(), c.slot.get(), c.bits.get(), c.sig.get(), n, 64, want.data(), t);
  uint32_t bad = n;
  for (uint32_t i = n; i-- > 0;)
    if (cls[i] != want[i]) bad = i;
  CHECK(bad == n, "%s, %u rows, %u hash bits: row %u has class %u, dedup_classes gives %u", what, n, hash_bits, bad,
        bad < n ? cls[bad] : 0, bad < n ? want[bad] : 0);
  ++n_batches;
  n_rows += n;
}

static void functor_checks() {
  const uint32_t widths[4] = {64, 7, 1, 0};
  for (uint32_t n = 1; n <= 200; ++n) {
    Columns c(n);
    const uint32_t distinct = 1 + (uint32_t)rnd(n);  // rows 0 .. distinct-1 random; the rest copies, some off by a bit
    for (uint32_t i = 0; i < n; ++i) {
      if (i < distinct) {
        c.random_row(i);
        continue;
      }
      c.copy_row(i, (uint32_t)rnd(i));
      if (rnd(4) == 0) *c.byte(i, (uint32_t)rnd(280)) ^= (uint8_t)(1u << rnd(8));
    }
    for (uint32_t w : widths) classify_check(c, w, "seeded batch");
  }
  Columns flip(281);
  flip.random_row(0);
  for (uint32_t k = 0; k < 280; ++k) {
    flip.copy_row(1 + k, 0);
    *flip.byte(1 + k, k) ^= (uint8_t)(1u << (k % 8));
  }
  for (uint32_t w : widths) classify_check(flip, w, "flip table");
}

// ---- (b) the allocations of the two entries
static std::vector<Scenario> scenarios() {
  std::vector<Scenario> v;
  auto nothing = [](lcv_ctx*) { return (int)LCV_OK; };
  v.push_back({"lcv_batch_classify", nothing, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(3);
    zb.slot[1] = 5;  // two classes
    const uint32_t six[3] = {1, 0, 1};
    lcv_dbatch* db = nullptr;
    LCV_TRY(lcv_batch_upload_stores(c, &zb.hb, six, &db));
    uint64_t classes = 77;
    uint32_t cls[3] = {0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu};
    int rc = lcv_batch_classify(c, db, &classes);
    if (rc == LCV_OK) rc = lcv_debug_batch_classes(c, db, cls);
    lcv_batch_free(c, db);
    put(o, &classes, 1);
    put(o, cls, 3);
    return rc;
  }});
  v.push_back({"lcv_batch_classify + lcv_batch_fan_out (rows, stores) + lcv_batch_download", nothing, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(2);
    zb.slot[1] = 9;
    lcv_dbatch* db = nullptr;
    lcv_dbatch* fan = nullptr;
    LCV_TRY(lcv_batch_upload(c, &zb.hb, &db));
    uint64_t classes = 0;
    const uint32_t rows[3] = {1, 0, 1}, six[3] = {0, 1, 1};
    uint32_t cls[3] = {0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu};
    OutBatch ob(3, 1);
    int rc = lcv_batch_classify(c, db, &classes);
    if (rc == LCV_OK) rc = lcv_batch_fan_out(c, db, rows, six, 3, &fan);
    if (rc == LCV_OK) rc = lcv_debug_batch_classes(c, fan, cls);
    if (rc == LCV_OK) rc = lcv_batch_download(c, fan, nullptr, 0, &ob.hb);
    lcv_batch_free(c, fan);
    lcv_batch_free(c, db);
    put(o, cls, 3);
    ob.append_to(o);
    return rc;
  }});
  v.push_back({"lcv_batch_fan_out (identity, stores), unclassed", nothing, [](lcv_ctx* c, Bytes& o) {
    ZeroBatch zb(2);
    lcv_dbatch* db = nullptr;
    lcv_dbatch* fan = nullptr;
    LCV_TRY(lcv_batch_upload(c, &zb.hb, &db));
    const uint32_t six[2] = {1, 0};
    uint64_t shape[2] = {0, 0};
    int rc = lcv_batch_fan_out(c, db, nullptr, six, 2, &fan);
    if (rc == LCV_OK) rc = lcv_batch_shape(c, fan, &shape[0], &shape[1]);
    lcv_batch_free(c, fan);
    lcv_batch_free(c, db);
    put(o, shape, 2);
    return rc;
  }});
  return v;
}

// the two entries alone, on a batch made beforehand: what host_sweep fails are THEIR host allocations
static lcv_dbatch* g_db = nullptr;
static int upload_zero(lcv_ctx* c) {
  ZeroBatch zb(3);
  const uint32_t six[3] = {0, 1, 0};
  return lcv_batch_upload_stores(c, &zb.hb, six, &g_db);
}
static void free_zero(lcv_ctx* c) {
  lcv_batch_free(c, g_db);
  g_db = nullptr;
}
static std::vector<Scenario> host_scenarios() {
  std::vector<Scenario> v;
  v.push_back({"lcv_batch_classify (host allocations)", upload_zero, [](lcv_ctx* c, Bytes&) {
    uint64_t classes = 0;
    return lcv_batch_classify(c, g_db, &classes);
  }, free_zero});
  v.push_back({"lcv_batch_fan_out of a classed batch (host allocations)", [](lcv_ctx* c) {
    uint64_t classes = 0;
    LCV_TRY(upload_zero(c));
    return lcv_batch_classify(c, g_db, &classes);
  }, [](lcv_ctx* c, Bytes&) {
    const uint32_t rows[2] = {2, 0}, six[2] = {1, 1};
    lcv_dbatch* fan = nullptr;
    const int rc = lcv_batch_fan_out(c, g_db, rows, six, 2, &fan);
    lcv_batch_free(c, fan);
    return rc;
  }, free_zero});
  return v;
}

int main() {
  functor_checks();
  printf("dedup_class_check: functors: %llu batches, %llu rows, %llu confirm launches, %llu pairs\n", n_batches, n_rows,
         n_confirm_launches, n_pairs);
  for (const Scenario& s : scenarios()) sweep(s);
  // classify: the key, signature_slot, class, store and pair vectors; fan-out: the three inherited columns and the batch
  const long expect[2] = {4, 3};
  int k = 0;
  for (const Scenario& s : host_scenarios()) host_sweep(s, expect[k++]);
  printf("dedup_class_check: %llu scenarios, %llu device or pinned injections, %llu host injections, %llu failures\n",
         n_scenarios, n_injections, n_host_injections, failures);
  return failures ? 1 : 0;
}
