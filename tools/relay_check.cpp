// relay_check.cpp — stand-alone memory-safety and equivalence check of the asynchronous relay (lcv_relay_async) on its
// host path, meant to be built with sanitizers.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -pthread -fopenmp -DLCV_ALLOC_CHECK -Wl,--wrap=_Znwm -Wl,--wrap=_Znam -I light-client-consensus-specs_amd/build \
//       tools/relay_check.cpp light-client-consensus-specs_amd/csrc/lcv_wire.cpp -o relay_check && ./relay_check [mutations]
// (1) The kernel's functor (F_wire_relay, csrc/lcv_wire_dec.hpp: F_wire_dec's rounds through a row map) follows
//     offsets that a peer chose and a row map, so every round is run lane by lane over heap buffers of EXACTLY the
//     staged, LDS (pre-filled with garbage), meta, record, map and column sizes: an access one byte out of any of them
//     is a sanitizer report.  Every batch runs twice: over the staging buffer as the driver lays it out (16 zero bytes
//     behind the last message) and over one that ends where the last message's last 16-byte word does, so a load at or
//     past dev_off + round_up(len, 16) of the last message is a report too.  Inputs, for kinds 1 and 2 x every fork:
//     good messages of every extra_data length (among them last messages whose length is a multiple of 16, which end
//     exactly at the end of the tight buffer), the malformed table of tests/wire_decode_cases.py's shape, seeded
//     mutations of good messages (tools/wire_check_common.hpp), each with random pair lists (repeats, unnamed
//     messages, more pairs than messages and fewer).  Rows are compared with the host decoder's rows
//     (csrc/lcv_wire.cpp, linked) gathered by the map, statuses with its statuses; no record but the messages' and no
//     row but the pairs' may be written.
// (2) Through tools/driver_alloc_harness.hpp: every device and pinned allocation of lcv_relay_async + lcv_slot_wait_relay
//     (with lcv_set_dedup on and a fold) fails once — LCV_ENOMEM, then the same call succeeds with a fresh context's
//     outputs — every host allocation ahead of its first device allocation fails once (LCV_ENOMEM, no exception leaves
//     the library), and nothing is live after lcv_destroy.
// Prints its counts and `N failures`; exit status 1 on any.  No device, no library, nothing loaded into an interpreter.
#include "driver_alloc_harness.hpp"  // the host simulation: lcv_wire_dec.hpp and the driver among it
#include "wire_check_common.hpp"

static unsigned long long n_batches = 0, n_msgs = 0, n_pairs = 0, n_ok = 0, n_bad = 0, n_exact_end = 0;

// one batch through F_wire_relay as lcv_relay_async drives it, and through the host decoder
static void check_batch(const std::vector<Bytes>& msgs, const std::vector<uint8_t>& codes, const std::vector<uint32_t>& rows,
                        int kind, bool tight, const char* what) {
  using namespace lcv;
  const size_t n = msgs.size(), np = rows.size();
  size_t total = 0, staged = 0;
  for (const Bytes& m : msgs) { total += m.size(); staged += (m.size() + 15) & ~(size_t)15; }
  const size_t stage_bytes = staged + (tight ? 0 : 16);
  std::unique_ptr<uint8_t[]> buf(new uint8_t[total ? total : 1]), stage(new uint8_t[stage_bytes ? stage_bytes : 1]);
  std::unique_ptr<uint8_t[]> meta(new uint8_t[DEC_META_BYTES * n]), rec(new uint8_t[DEC_REC_BYTES * n]);
  std::unique_ptr<uint32_t[]> map(new uint32_t[np]);
  std::vector<uint64_t> offs(n), lens(n);
  memset(stage.get(), 0xA5, stage_bytes);
  size_t o = 0, so = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!msgs[i].empty()) {
      memcpy(buf.get() + o, msgs[i].data(), msgs[i].size());
      memcpy(stage.get() + so, msgs[i].data(), msgs[i].size());
    }
    offs[i] = o; lens[i] = msgs[i].size();
    const uint64_t at = so;
    const uint32_t len = (uint32_t)msgs[i].size(), f = codes[i];
    memcpy(meta.get() + DEC_META_BYTES * i, &at, 8);
    memcpy(meta.get() + DEC_META_BYTES * i + 8, &len, 4);
    memcpy(meta.get() + DEC_META_BYTES * i + 12, &f, 4);
    o += msgs[i].size();
    so += (msgs[i].size() + 15) & ~(size_t)15;
  }
  if (!tight) memset(stage.get() + so, 0, 16);
  if (tight && n && !msgs[n - 1].empty() && msgs[n - 1].size() % 16 == 0) ++n_exact_end;
  for (size_t i = 0; i < np; ++i) map[i] = rows[i];
  // the yardstick: the host decoder's rows of the messages
  Cols H = make_cols(n ? n : 1, 0x11);
  lcv_update_batch hb = {};
  hb.attested.beacon = H.c[0].get(); hb.attested.execution = H.c[1].get(); hb.attested.exec_branch = H.c[2].get();
  hb.finalized.beacon = H.c[3].get(); hb.finalized.execution = H.c[4].get(); hb.finalized.exec_branch = H.c[5].get();
  hb.nsc_index = H.nsc_index.get(); hb.nsc_branch = H.c[6].get(); hb.finality_branch = H.c[7].get();
  hb.sync_bits = H.c[8].get(); hb.sync_signature = H.c[9].get(); hb.signature_slot = H.slot.get();
  hb.n = n;
  std::vector<uint64_t> pool_src(n + 1);
  std::vector<uint8_t> hstatus(n);
  uint64_t hpool = 0;
  if (lcv_ssz_decode_updates_mixed(buf.get(), offs.data(), lens.data(), n, kind, codes.data(), &hb, pool_src.data(), &hpool,
                                   hstatus.data()) != LCV_OK) {
    CHECK(false, "%s: the host decoder refused the batch", what);
    return;
  }
  // the kernel: a team per pair, then a team per message
  Cols D = make_cols(np ? np : 1, 0xEE);
  memset(rec.get(), 0xEE, DEC_REC_BYTES * n);
  const ProdOut O = {D.c[0].get(), D.c[1].get(), D.c[2].get(), D.c[3].get(), D.c[4].get(), D.c[5].get(), D.nsc_index.get(),
                     D.c[6].get(), D.c[7].get(), D.c[8].get(), D.c[9].get(), D.slot.get()};
  const DecArgs A = {stage.get(), meta.get(), rec.get(), O, (uint32_t)kind, (uint32_t)DEC_ROWS};
  run_team(F_wire_relay{RelayDecArgs{A, map.get(), (uint32_t)np}}, (uint32_t)(np + n));
  for (size_t j = 0; j < n; ++j) {
    uint32_t st, one;
    memcpy(&st, rec.get() + DEC_REC_BYTES * j, 4);
    memcpy(&one, rec.get() + DEC_REC_BYTES * j + 4, 4);
    CHECK(st == hstatus[j] && one == 1u, "%s: message %zu (%zu bytes, fork %u): status %u (host %u), word 1 = %u", what, j,
          msgs[j].size(), codes[j], st, hstatus[j], one);
    (st ? n_bad : n_ok)++;
  }
  for (size_t i = 0; i < np; ++i) {
    const size_t s = rows[i];
    for (int k = 0; k < 10; ++k)
      CHECK(memcmp(D.c[k].get() + kWidth[k] * i, H.c[k].get() + kWidth[k] * s, kWidth[k]) == 0,
            "%s: pair %zu (message %zu): column %d differs", what, i, s, k);
    CHECK(D.slot[i] == H.slot[s], "%s: pair %zu (message %zu): signature_slot", what, i, s);
    CHECK(D.nsc_index[i] == 0, "%s: pair %zu: nsc_index written", what, i);
  }
  ++n_batches;
  n_msgs += n;
  n_pairs += np;
}

// pair lists over n messages: every message once; a random list (repeats, unnamed messages); one pair
static void check_lists(const std::vector<Bytes>& msgs, const std::vector<uint8_t>& codes, int kind, const char* what) {
  const uint32_t n = (uint32_t)msgs.size();
  std::vector<uint32_t> all(n), some(1 + rnd(2 * n + 3)), one(1, (uint32_t)rnd(n));
  for (uint32_t i = 0; i < n; ++i) all[i] = n - 1 - i;  // (descending)
  for (uint32_t& r : some) r = (uint32_t)rnd(n);
  for (int tight = 0; tight < 2; ++tight) {
    check_batch(msgs, codes, all, kind, tight != 0, what);
    check_batch(msgs, codes, some, kind, tight != 0, what);
    check_batch(msgs, codes, one, kind, tight != 0, what);
  }
}

static void functor_checks(unsigned long mutations) {
  for (int kind = 1; kind < 3; ++kind)
    for (int fork = 0; fork < 3; ++fork) {
      char what[64];
      // good messages: every extra_data length; each in turn the last message of the buffer
      std::vector<Bytes> msgs;
      for (uint32_t e = 0; e <= 32; ++e) msgs.push_back(good_message(kind, fork, e, (7 * e + 3) % 33));
      snprintf(what, sizeof what, "good %d/%d", kind, fork);
      check_lists(msgs, std::vector<uint8_t>(msgs.size(), (uint8_t)fork), kind, what);
      CHECK(n_bad == 0, "%s: a good message was refused", what);
      for (uint32_t e = 0; e <= 32; ++e) {
        const std::vector<Bytes> two = {good_message(kind, fork, 32, 32), good_message(kind, fork, e, (e + 8) % 33)};
        check_batch(two, {(uint8_t)fork, (uint8_t)fork}, {1, 0, 1}, kind, true, what);
      }
      // the table: each bad message between two good ones, and as the first and the last of a buffer
      const std::vector<Bytes> table = malformed_table(kind, fork);
      const Bytes good = good_message(kind, fork, 32, 32);
      msgs.assign(1, good);
      for (const Bytes& b : table) { msgs.push_back(b); msgs.push_back(good); }
      snprintf(what, sizeof what, "table %d/%d", kind, fork);
      const unsigned long long bad0 = n_bad;
      check_batch(msgs, std::vector<uint8_t>(msgs.size(), (uint8_t)fork), {0}, kind, false, what);
      CHECK(n_bad - bad0 == table.size(), "%s: %llu of %zu table entries refused", what, n_bad - bad0, table.size());
      check_lists(msgs, std::vector<uint8_t>(msgs.size(), (uint8_t)fork), kind, what);
      for (const Bytes& b : table) {
        check_lists({b, good}, {(uint8_t)fork, (uint8_t)fork}, kind, what);
        check_lists({good, b}, {(uint8_t)fork, (uint8_t)fork}, kind, what);
      }
      n_bad = 0;
    }
  n_ok = 0;
  for (int kind = 1; kind < 3; ++kind)
    for (int fork = 0; fork < 3; ++fork)
      for (unsigned long done = 0; done < mutations; done += 8) {
        std::vector<Bytes> msgs;
        std::vector<uint8_t> codes;
        for (int j = 0; j < 8; ++j) {
          uint8_t code;
          msgs.push_back(mutate(kind, fork, &code));
          codes.push_back(code);
        }
        char what[64];
        snprintf(what, sizeof what, "mutations %d/%d at %lu", kind, fork, done);
        check_lists(msgs, codes, kind, what);
      }
  CHECK(n_exact_end > 0, "no last message ended exactly at the end of the staged buffer");
}

// ---- (2) the driver's allocations
static int relay_call(lcv_ctx* c, Bytes& o) {
  // two Altair-format finality messages (fixed size), all zero; three pairs over the harness's two stores
  const uint64_t len = 112 + 112 + 192 + 168, offs[2] = {0, 16}, lens[2] = {len, len};
  const uint32_t rows[3] = {0, 1, 1}, six[3] = {1, 0, 1};
  lcv_fold_state in[2];
  lcv_fold_result res[2];
  memset(in, 0, sizeof in);
  memset(res, 0xEE, sizeof res);
  lcv_relay_request rq = {};
  rq.buf = kZero.data(); rq.buf_len = kZero.size(); rq.offsets = offs; rq.lengths = lens; rq.nmsg = 2;
  rq.kind = 1; rq.fork = 2; rq.forks = nullptr; rq.rows = rows; rq.store_index = six; rq.npairs = 3;
  rq.current_slot = kNow; rq.genesis_validators_root = kGvr; rq.fold_in = in;
  uint8_t out[2 + 3 + 3];
  memset(out, 0xEE, sizeof out);
  LCV_TRY(lcv_relay_async(c, &rq, 2));
  LCV_TRY(lcv_slot_wait_relay(c, 2, out, out + 2, out + 5, res));
  uint64_t dd[2] = {0, 0};
  LCV_TRY(lcv_last_dedup(c, 2, &dd[0], &dd[1]));
  put(o, out, sizeof out);
  put(o, res, 2);
  put(o, dd, 2);
  return LCV_OK;
}

int main(int argc, char** argv) {
  const unsigned long mutations = argc > 1 ? strtoul(argv[1], nullptr, 10) : 600;
  functor_checks(mutations);
  const Scenario plain = {"lcv_relay_async + lcv_slot_wait_relay", [](lcv_ctx* c) { return set_table(c); }, relay_call, nullptr};
  const Scenario modes = {"lcv_relay_async under lcv_set_dedup, latency mode off", [](lcv_ctx* c) {
    LCV_TRY(set_table(c));
    LCV_TRY(lcv_set_latency_mode(c, 0));
    return lcv_set_dedup(c, 1);
  }, relay_call, nullptr};
  sweep(plain);
  sweep(modes);
  host_sweep(modes, 6);  // the grouping by store, the messages' tuples and classes, the pairs' items
  printf("relay_check: %llu batches, %llu messages, %llu pairs (mutated: %llu accepted, %llu refused), %llu exact ends, "
         "%llu scenarios, %llu device or pinned injections, %llu host injections, %llu failures\n", n_batches, n_msgs, n_pairs,
         n_ok, n_bad, n_exact_end, n_scenarios, n_injections, n_host_injections, failures);
  return failures ? 1 : 0;
}
