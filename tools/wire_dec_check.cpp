// wire_dec_check.cpp — stand-alone memory-safety and equivalence check of the device SSZ decoder's kernels
// (csrc/lcv_wire_dec.hpp: F_wire_dec, F_sc_confirm, F_sc_gather) on their host path, meant to be built with sanitizers.
// The kernels follow offsets that a peer chose, so every round of every functor is run lane by lane over heap buffers
// of EXACTLY the staged, LDS, record and column sizes: an access one byte out of any of them is a sanitizer report.
// The rows, statuses and committees are compared with the host decoder (csrc/lcv_wire.cpp, included here).  Both
// decoders take the containers and the acceptance rule from csrc/lcv_wire_layout.hpp, so their agreement says nothing
// about the layout: this program checks memory safety and that malformed messages (built below from literal sizes of
// its own) are refused.  The layout is pinned by the reference-serialised bytes of tests/golden/wire.npz and by
// tests/wire_layout_cases.py, which share nothing with that header.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -pthread -DLCV_HOSTSIM=1 -I light-client-consensus-specs_amd/csrc \
//       tools/wire_dec_check.cpp -o wire_dec_check && ./wire_dec_check [mutations per kind and fork, default 1500]
// Inputs, for every kind x fork: good messages (every extra_data length 0 .. 32, so the finalized header starts at
// every residue modulo 16); the table of malformed messages of tests/wire_decode_cases.py; and seeded random mutations
// of good messages — truncations, extensions, 32-bit writes at the offset positions (boundary values: 0, the fixed
// size and the length +- 1, 0x80000000, 0xFFFFFFFF ...) and at random positions, a zeroed committee, fork codes 0 .. 3.
// The bytes between a message's end and the next 16-byte boundary of the staging buffer are filled with 0xA5.
// Prints its counts; exit status 1 on any difference.  No device, no library, nothing loaded into an interpreter.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <memory>
#include <random>
#include <string>

#define LCV_HD
#include "lcv_dedup_plan.hpp"  // dedup_truncate
#include "lcv_wire_dec.hpp"

#include "lcv_wire.cpp"  // the yardstick: lcv_ssz_decode_updates_mixed

#include "wire_check_common.hpp"

static unsigned long long n_batches = 0, n_msgs = 0, n_ok = 0, n_bad = 0, n_confirm = 0, n_pool = 0, failures = 0;
#define CHECK(x, ...)                                                      \
  do {                                                                     \
    if (!(x)) {                                                            \
      printf("FAILED %s (line %d): ", #x, __LINE__);                       \
      printf(__VA_ARGS__);                                                 \
      printf("\n");                                                        \
      if (++failures > 20) exit(1);                                        \
    }                                                                      \
  } while (0)

// one batch through the three functors as lcv_batch_decode drives them, and through the host decoder
static void check_batch(const std::vector<Bytes>& msgs, const std::vector<uint8_t>& codes, int kind, uint32_t hash_bits,
                        const char* what) {
  using namespace lcv;
  const size_t n = msgs.size();
  // the caller's buffer (host decoder) and the staging scratch, both exact
  size_t total = 0, staged = 16;
  for (const Bytes& m : msgs) { total += m.size(); staged += (m.size() + 15) & ~(size_t)15; }
  std::unique_ptr<uint8_t[]> buf(new uint8_t[total ? total : 1]), stage(new uint8_t[staged]);
  std::unique_ptr<uint8_t[]> meta(new uint8_t[DEC_META_BYTES * n]), rec(new uint8_t[DEC_REC_BYTES * n]);
  std::vector<uint64_t> offs(n), lens(n), soff(n);
  memset(stage.get(), 0xA5, staged);
  size_t o = 0, so = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!msgs[i].empty()) {
      memcpy(buf.get() + o, msgs[i].data(), msgs[i].size());
      memcpy(stage.get() + so, msgs[i].data(), msgs[i].size());
    }
    offs[i] = o; lens[i] = msgs[i].size(); soff[i] = so;
    const uint32_t len = (uint32_t)msgs[i].size(), f = codes[i];
    memcpy(meta.get() + DEC_META_BYTES * i, &soff[i], 8);
    memcpy(meta.get() + DEC_META_BYTES * i + 8, &len, 4);
    memcpy(meta.get() + DEC_META_BYTES * i + 12, &f, 4);
    o += msgs[i].size();
    so += (msgs[i].size() + 15) & ~(size_t)15;
  }
  memset(stage.get() + so, 0, 16);
  // the yardstick
  Cols H = make_cols(n, 0x11);
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
  // the kernels
  Cols D = make_cols(n, 0xEE);
  DecArgs A = {stage.get(), meta.get(), rec.get(), ProdOut{}, (uint32_t)kind, (uint32_t)DEC_PLAN};
  memset(rec.get(), 0xEE, DEC_REC_BYTES * n);
  if (kind == 0) run_team(F_wire_dec{A}, (uint32_t)n);
  std::vector<uint8_t> rec1(rec.get(), rec.get() + DEC_REC_BYTES * n);
  A.O = ProdOut{D.c[0].get(), D.c[1].get(), D.c[2].get(), D.c[3].get(), D.c[4].get(), D.c[5].get(), D.nsc_index.get(),
                D.c[6].get(), D.c[7].get(), D.c[8].get(), D.c[9].get(), D.slot.get()};
  A.phase = DEC_ROWS;
  run_team(F_wire_dec{A}, (uint32_t)n);
  // the pool: groups by (truncated) hash, confirmed pair by pair
  const uint64_t none = DEC_NO_COMMITTEE;
  std::vector<uint64_t> coff(n, none), dpool;
  std::vector<uint32_t> dindex(n, 0);
  std::map<uint64_t, std::vector<uint32_t>> groups;  // hash -> pool rows
  int64_t zero_ix = -1;
  for (size_t i = 0; i < n; ++i) {
    uint32_t st, st1 = 0, zero = 1;
    uint64_t h = 0;
    memcpy(&st, rec.get() + DEC_REC_BYTES * i, 4);
    if (kind == 0) {
      memcpy(&st1, &rec1[DEC_REC_BYTES * i], 4);
      memcpy(&zero, &rec1[DEC_REC_BYTES * i + 4], 4);
      memcpy(&h, &rec1[DEC_REC_BYTES * i + 8], 8);
      CHECK(st1 == st, "%s: message %zu: the two passes disagree (%u, %u)", what, i, st1, st);
    }
    CHECK(st == hstatus[i], "%s: message %zu (%zu bytes, fork %u): status %u, host %u", what, i, msgs[i].size(), codes[i], st, hstatus[i]);
    (st ? n_bad : n_ok)++;
    if (st || zero) {
      if (zero_ix < 0) { zero_ix = (int64_t)dpool.size(); dpool.push_back(none); }
      dindex[i] = (uint32_t)zero_ix;
      continue;
    }
    coff[i] = soff[i] + (codes[i] == 2 ? 112 : 4);
    std::vector<uint32_t>& g = groups[dedup_truncate(h, hash_bits)];
    int64_t hit = -1;
    for (uint32_t p : g) {
      std::unique_ptr<uint8_t[]> pair(new uint8_t[DEC_PAIR_BYTES]);
      std::unique_ptr<uint32_t[]> differ(new uint32_t[1]);
      memcpy(pair.get(), &coff[i], 8);
      memcpy(pair.get() + 8, &dpool[p], 8);
      run_team(F_sc_confirm{ScConfirmArgs{stage.get(), pair.get(), differ.get()}}, 1);
      ++n_confirm;
      if (!differ[0]) { hit = p; break; }
    }
    if (hit < 0) { hit = (int64_t)dpool.size(); g.push_back((uint32_t)hit); dpool.push_back(coff[i]); }
    dindex[i] = (uint32_t)hit;
  }
  std::unique_ptr<uint8_t[]> pool(new uint8_t[(size_t)K_SC * dpool.size()]);
  memset(pool.get(), 0xEE, (size_t)K_SC * dpool.size());
  run_team(F_sc_gather{ScGatherArgs{stage.get(), dpool.data(), pool.get()}}, (uint32_t)dpool.size());
  n_pool += dpool.size();
  // rows, slots and committees
  for (int k = 0; k < 10; ++k)
    CHECK(memcmp(D.c[k].get(), H.c[k].get(), kWidth[k] * n) == 0, "%s: column %d differs", what, k);
  for (size_t i = 0; i < n; ++i) {
    CHECK(D.slot[i] == H.slot[i], "%s: signature_slot of row %zu", what, i);
    const uint64_t hs = pool_src[H.nsc_index[i]];
    const uint8_t* mine = pool.get() + (size_t)K_SC * dindex[i];
    if (hs == UINT64_MAX) CHECK(all_zero(mine, K_SC), "%s: row %zu: committee not zero", what, i);
    else CHECK(memcmp(mine, buf.get() + hs, K_SC) == 0, "%s: row %zu: committee differs", what, i);
  }
  CHECK(dpool.size() == hpool || hash_bits != 64, "%s: %zu pool rows, host %llu", what, dpool.size(), (unsigned long long)hpool);
  ++n_batches;
  n_msgs += n;
}

int main(int argc, char** argv) {
  const unsigned long mutations = argc > 1 ? strtoul(argv[1], nullptr, 10) : 1500;
  for (int kind = 0; kind < 3; ++kind)
    for (int fork = 0; fork < 3; ++fork) {
      char what[64];
      // good messages: every extra_data length, the finalized header at every residue
      std::vector<Bytes> msgs;
      for (uint32_t e = 0; e <= 32; ++e) msgs.push_back(good_message(kind, fork, e, (7 * e + 3) % 33));
      snprintf(what, sizeof what, "good %d/%d", kind, fork);
      check_batch(msgs, std::vector<uint8_t>(msgs.size(), (uint8_t)fork), kind, 64, what);
      if (n_bad) { printf("FAILED: a good message was refused (%s)\n", what); return 1; }
      // the table: each bad message between two good ones, and as the first and the last of a buffer
      const std::vector<Bytes> table = malformed_table(kind, fork);
      const Bytes good = good_message(kind, fork, 32, 32);
      const unsigned long long bad0 = n_bad;
      msgs.assign(1, good);
      for (const Bytes& b : table) { msgs.push_back(b); msgs.push_back(good); }
      snprintf(what, sizeof what, "table %d/%d", kind, fork);
      check_batch(msgs, std::vector<uint8_t>(msgs.size(), (uint8_t)fork), kind, 64, what);
      CHECK(n_bad - bad0 == table.size(), "%s: %llu of %zu table entries refused", what, n_bad - bad0, table.size());
      for (const Bytes& b : table) {
        check_batch({b, good}, {(uint8_t)fork, (uint8_t)fork}, kind, 64, what);
        check_batch({good, b}, {(uint8_t)fork, (uint8_t)fork}, kind, 64, what);
      }
      n_bad = 0;
    }
  n_ok = 0;
  // mutations, in batches of 8, a repeated and a zeroed committee among them; whole, one-bit and no hash
  for (int kind = 0; kind < 3; ++kind)
    for (int fork = 0; fork < 3; ++fork)
      for (unsigned long done = 0; done < mutations; done += 8) {
        std::vector<Bytes> msgs;
        std::vector<uint8_t> codes;
        for (int j = 0; j < 8; ++j) {
          uint8_t code;
          msgs.push_back(mutate(kind, fork, &code));
          codes.push_back(code);
        }
        if (kind == 0 && fork != 2 && msgs[0].size() > 4 + 24624 && msgs[5].size() > 4 + 24624)
          memcpy(&msgs[5][4], &msgs[0][4], 24624 - (rnd(3) ? 0 : 1));  // the same committee, or all but its last byte
        char what[64];
        snprintf(what, sizeof what, "mutations %d/%d at %lu", kind, fork, done);
        check_batch(msgs, codes, kind, done % 24 == 8 ? 1 : done % 24 == 16 ? 0 : 64, what);
      }
  printf("wire_dec_check: %llu batches, %llu messages (mutated: %llu accepted, %llu refused), %llu committee compares, "
         "%llu pool rows, %llu failures\n", n_batches, n_msgs, n_ok, n_bad, n_confirm, n_pool, failures);
  return failures ? 1 : 0;
}
