// driver_alloc_check.cpp — stand-alone check of the driver's memory handling (csrc/lcv_driver.inc: DevBuf, PinBuf,
// Scratch, batch_new, the boundary `guarded`) on the host simulation, meant to be built with sanitizers.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -pthread -fopenmp -DLCV_ALLOC_CHECK -Wl,--wrap=_Znwm -Wl,--wrap=_Znam -I light-client-consensus-specs_amd/build \
//       tools/driver_alloc_check.cpp light-client-consensus-specs_amd/csrc/lcv_wire.cpp -o driver_alloc_check
// It includes the host simulation, whose LCV_ALLOC_CHECK hook counts the live device and pinned allocations and fails
// the k-th allocation on request (through tools/driver_alloc_harness.hpp, which holds the sweeps and the failing
// operator new and which tools/dedup_class_check.cpp shares).
// (a) For every scenario below, and k = 0, 1, 2, ... until the call makes fewer than k + 1 device or pinned
//     allocations: on a fresh context, with allocation k of the call failing, the call returns LCV_ENOMEM with a
//     message; the same call again, with nothing failing, succeeds; and its outputs equal those of a fresh context on
//     which nothing ever failed.  The batches have at most 2 all-zero rows: the allocation paths do not depend on
//     what the rows hold.  The "used slot" scenarios start from a slot that holds a finished 1-row batch of the same
//     entry, so that the call regrows all three buffers of the slot's HostSlot; between the failure and the retry every
//     wait is called on the slot: the failed enqueue left no results (lcv_slot_wait reads the work space, LCV_OK; the
//     other three waits LCV_ESTATE), and no wait reads a buffer that the failed call released.
// (b) With a replacement operator new that throws std::bad_alloc on its n-th call on this thread: every host
//     allocation that lcv_set_store_table and lcv_fast_aggregate_verify (3 keys) make ahead of their first device
//     allocation fails once; each call returns LCV_ENOMEM, and no exception leaves the library.
// (c) After lcv_destroy no device or pinned allocation is live (and LeakSanitizer reports nothing at exit).
// Prints its counts; exit status 1 on any failure.  No device, no library, nothing loaded into an interpreter.
#include "driver_alloc_harness.hpp"

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

// ---- a slot in use (slot 1): the four host-input entries with n rows (the relay: n messages, n pairs) and their waits
static int used_async(lcv_ctx* c, int n, Bytes& o) {
  ZeroBatch zb(n);
  uint8_t out[4] = {0xEE, 0xEE, 0xEE, 0xEE};
  LCV_TRY(lcv_validate_async(c, &zb.hb, kNow, kGvr, 1));
  LCV_TRY(lcv_slot_wait(c, 1, n, out, out + 2));
  put(o, out, 4);
  return LCV_OK;
}
static int used_async_fold(lcv_ctx* c, int n, Bytes& o) {
  ZeroBatch zb(n);
  lcv_fold_state in;
  lcv_fold_result res;
  memset(&in, 0, sizeof in);
  memset(&res, 0xEE, sizeof res);
  uint8_t out[4] = {0xEE, 0xEE, 0xEE, 0xEE};
  LCV_TRY(lcv_validate_async_fold(c, &zb.hb, kNow, kGvr, &in, 1));
  LCV_TRY(lcv_slot_wait_fold(c, 1, n, out, out + 2, &res));
  put(o, out, 4);
  put(o, &res, 1);
  return LCV_OK;
}
static int used_stores_async_fold(lcv_ctx* c, int n, Bytes& o) {
  ZeroBatch zb(n);
  const uint32_t six[2] = {1, 0};
  lcv_fold_state in[2];
  lcv_fold_result res[2];
  memset(in, 0, sizeof in);
  memset(res, 0xEE, sizeof res);
  uint8_t out[4] = {0xEE, 0xEE, 0xEE, 0xEE};
  LCV_TRY(lcv_validate_stores_async_fold(c, &zb.hb, six, kNow, kGvr, in, 1));
  LCV_TRY(lcv_slot_wait_stores_fold(c, 1, n, out, out + 2, res));
  put(o, out, 4);
  put(o, res, 2);
  return LCV_OK;
}
static int used_relay(lcv_ctx* c, int n, Bytes& o) {
  // Altair-format finality messages (fixed size), all zero; a pair per message over the harness's two stores
  const uint64_t len = 112 + 112 + 192 + 168, offs[2] = {0, 16}, lens[2] = {len, len};
  const uint32_t rows[2] = {0, 1}, six[2] = {1, 0};
  lcv_fold_state in[2];
  lcv_fold_result res[2];
  memset(in, 0, sizeof in);
  memset(res, 0xEE, sizeof res);
  lcv_relay_request rq = {};
  rq.buf = kZero.data(); rq.buf_len = kZero.size(); rq.offsets = offs; rq.lengths = lens; rq.nmsg = n;
  rq.kind = 1; rq.fork = 2; rq.forks = nullptr; rq.rows = rows; rq.store_index = six; rq.npairs = n;
  rq.current_slot = kNow; rq.genesis_validators_root = kGvr; rq.fold_in = in;
  uint8_t out[6] = {0xEE, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE};
  LCV_TRY(lcv_relay_async(c, &rq, 1));
  LCV_TRY(lcv_slot_wait_relay(c, 1, out, out + 2, out + 4, res));
  put(o, out, 6);
  put(o, res, 2);
  return LCV_OK;
}
// every wait on slot 1 after a failed enqueue: the slot holds no results, and its work space (64 rows from the
// prepared batch) is what lcv_slot_wait reads
static void waits_on_failed_slot(lcv_ctx* c, const char* name, long k) {
  uint8_t st[2], vr[2];
  lcv_fold_result res[2];
  const int w = lcv_slot_wait(c, 1, 1, vr, vr + 1), wf = lcv_slot_wait_fold(c, 1, 1, vr, vr + 1, res),
            ws = lcv_slot_wait_stores_fold(c, 1, 1, vr, vr + 1, res), wr = lcv_slot_wait_relay(c, 1, st, vr, vr + 1, nullptr),
            wrf = lcv_slot_wait_relay(c, 1, st, vr, vr + 1, res);
  CHECK(w == LCV_OK && wf == LCV_ESTATE && ws == LCV_ESTATE && wr == LCV_ESTATE && wrf == LCV_ESTATE,
        "%s: after allocation %ld failed, the waits returned %d %d %d %d %d", name, k, w, wf, ws, wr, wrf);
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
  struct Used { const char* name; int (*prep)(lcv_ctx*); int (*run)(lcv_ctx*, int, Bytes&); };
  const Used used[] = {
      {"lcv_validate_async on a used slot", set_store, used_async},
      {"lcv_validate_async_fold on a used slot", set_store, used_async_fold},
      {"lcv_validate_stores_async_fold on a used slot", [](lcv_ctx* c) { return set_table(c); }, used_stores_async_fold},
      {"lcv_relay_async on a used slot", [](lcv_ctx* c) { return set_table(c); }, used_relay},
  };
  for (const Used& u : used)
    v.push_back({u.name, [u](lcv_ctx* c) { Bytes o; LCV_TRY(u.prep(c)); return u.run(c, 1, o); },
                 [u](lcv_ctx* c, Bytes& o) { return u.run(c, 2, o); }, nullptr, waits_on_failed_slot,
                 3});  // (the pinned region, the results region and the device copy all regrow)
  return v;
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
