// wire_check_common.hpp — what the stand-alone checks of the device SSZ decoder share (tools/wire_dec_check.cpp,
// tools/relay_check.cpp): the message generators — good messages from literal sizes of their own, the table of malformed
// messages of tests/wire_decode_cases.py, seeded mutations — a team launch run lane by lane over a heap LDS block of
// exactly the functor's size, and exact-size heap columns.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

typedef std::vector<uint8_t> Bytes;
static std::mt19937_64 rng(0x6c6376u);
static uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }

static void put32(Bytes& b, size_t pos, uint32_t v) {
  if (pos + 4 <= b.size()) memcpy(&b[pos], &v, 4);
}
static void app32(Bytes& b, uint32_t v) { b.insert(b.end(), (uint8_t*)&v, (uint8_t*)&v + 4); }
static void app_rand(Bytes& b, size_t n) {
  for (size_t k = 0; k < n; ++k) b.push_back((uint8_t)(1 + rnd(255)));
}

static const uint32_t kFixed[3] = {25152, 368, 172};
static uint32_t exec_fixed(int fork) { return fork == 0 ? 584 : 568; }

static Bytes good_header(int fork, uint32_t elen) {
  Bytes h;
  app_rand(h, 112);
  app32(h, 244);
  app_rand(h, 128);
  const size_t e = h.size();
  app_rand(h, exec_fixed(fork));
  put32(h, e + 436, exec_fixed(fork));
  app_rand(h, elen);
  return h;
}
static Bytes good_message(int kind, int fork, uint32_t elen_att, uint32_t elen_fin) {
  Bytes m;
  if (fork == 2) {
    app_rand(m, 112);
    if (kind == 0) app_rand(m, 24624 + 160);
    if (kind <= 1) app_rand(m, 112 + 192);
    app_rand(m, 168);
    return m;
  }
  const Bytes att = good_header(fork, elen_att), fin = good_header(fork, elen_fin);
  app32(m, kFixed[kind]);
  if (kind == 0) app_rand(m, 24624 + 160);
  if (kind <= 1) {
    app32(m, kFixed[kind] + (uint32_t)att.size());
    app_rand(m, 192);
  }
  app_rand(m, 168);
  m.insert(m.end(), att.begin(), att.end());
  if (kind <= 1) m.insert(m.end(), fin.begin(), fin.end());
  return m;
}

// ---- the malformed table (tests/wire_decode_cases.py malformed_table)
static std::vector<Bytes> malformed_table(int kind, int fork) {
  const Bytes good = good_message(kind, fork, 32, 32);
  const uint32_t n = (uint32_t)good.size();
  std::vector<Bytes> t;
  auto cut = [&](size_t len) { t.push_back(Bytes(good.begin(), good.begin() + len)); };
  auto w32 = [&](size_t pos, uint32_t v) { Bytes b = good; put32(b, pos, v); t.push_back(b); };
  auto ext = [&](uint8_t v) { Bytes b = good; b.push_back(v); t.push_back(b); };
  t.push_back(Bytes());
  if (fork == 2) {
    cut(n - 1);
    ext(0);
    return t;
  }
  const uint32_t fixed = kFixed[kind], ef = exec_fixed(fork), hdr = 244 + ef + 32;
  const size_t pos2 = kind == 0 ? 4 + 24624 + 160 : 4;
  cut(fixed - 1);
  cut(fixed);
  w32(0, fixed + 1);
  w32(0, fixed - 1);
  w32(fixed + 112, 245);
  w32(fixed + 244 + 436, ef + 4);
  ext(7);
  ext(0);
  if (kind <= 1) {
    for (uint32_t v : {fixed - 1, n + 1, 0x80000000u, 0xFFFFFFFFu, n, fixed + 243, fixed + 244 + ef - 1, fixed + hdr + 1}) w32(pos2, v);
    cut(fixed + hdr + 243);
    cut(fixed + hdr + 244 + ef - 1);
    w32(fixed + hdr + 112, 243);
    w32(fixed + hdr + 244 + 436, ef - 1);
  } else {
    cut(fixed + 243);
    cut(fixed + 244 + ef - 1);
  }
  return t;
}

// ---- a seeded mutation of a good message
static Bytes mutate(int kind, int fork, uint8_t* code) {
  Bytes m = good_message(kind, fork, (uint32_t)rnd(33), (uint32_t)rnd(33));
  const uint32_t n = (uint32_t)m.size(), fixed = fork == 2 ? n : kFixed[kind], ef = exec_fixed(fork);
  *code = (uint8_t)fork;
  const size_t pos2 = kind == 0 ? 4 + 24624 + 160 : 4;
  uint32_t a1 = n;
  if (fork != 2 && kind <= 1) memcpy(&a1, &m[pos2], 4);
  const size_t spots[6] = {0, pos2, (size_t)fixed + 112, (size_t)fixed + 244 + 436, (size_t)a1 + 112, (size_t)a1 + 244 + 436};
  const uint32_t values[] = {0, 1, 3, 4, n, n - 1, n + 1, fixed, fixed - 1, fixed + 1, a1 - 1, a1 + 1, fixed + 243, fixed + 244,
                             fixed + 244 + ef, fixed + 244 + ef - 1, 243, 244, 245, ef, ef - 1, ef + 1, 0x80000000u, 0xFFFFFFFFu,
                             0x7FFFFFFFu, 0x80000000u + fixed, 0xFFFFFFF0u, (uint32_t)rng()};
  const size_t nvalues = sizeof(values) / sizeof(values[0]);
  switch (rnd(8)) {
    case 0: m.resize(rnd(n + 1)); break;                                     // truncation, anywhere
    case 1: m.resize(n - 1 - rnd(n < 40 ? n - 1 : 40)); break;               // ... near the end
    case 2: m.resize(fixed > 20 ? fixed - 20 + rnd(300) : rnd(300)); break;  // ... around the fixed part
    case 3: app_rand(m, 1 + rnd(70)); break;                                 // extension
    case 4: case 5: put32(m, spots[rnd(6)], values[rnd(nvalues)]); break;    // an offset field
    case 6: put32(m, rnd(n), rnd(2) ? values[rnd(nvalues)] : (uint32_t)rng()); break;
    default:
      if (kind == 0 && rnd(2)) memset(&m[fork == 2 ? 112 : 4], 0, 24624);    // SyncCommittee()
      else *code = (uint8_t)rnd(4);                                          // another fork's layout, or no fork
  }
  if (rnd(6) == 0) put32(m, spots[rnd(6)], values[rnd(nvalues)]);            // sometimes two at once
  return m;
}

// ---- a team launch, lane by lane, the LDS area a heap block of exactly F::LDS_WORDS words
template <class F> static void run_team(const F& f, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    std::unique_ptr<uint32_t[]> lds(new uint32_t[F::LDS_WORDS]);
    for (uint32_t k = 0; k < F::LDS_WORDS; ++k) lds[k] = 0xDEADBEEFu;  // (no round may rely on a cleared LDS)
    const uint32_t R = f.rounds();
    for (uint32_t r = 0; r < R; ++r)
      for (uint32_t lane = 0; lane < F::TEAM; ++lane) f(i, lane, r, lds.get(), nullptr);
  }
}

struct Cols {
  std::unique_ptr<uint8_t[]> c[10];
  std::unique_ptr<uint32_t[]> nsc_index;
  std::unique_ptr<uint64_t[]> slot;
};
static const size_t kWidth[10] = {112, 832, 128, 112, 832, 128, 160, 192, 64, 96};
static Cols make_cols(size_t n, uint8_t fill) {
  Cols C;
  for (int k = 0; k < 10; ++k) {
    C.c[k].reset(new uint8_t[kWidth[k] * n]);
    memset(C.c[k].get(), fill, kWidth[k] * n);
  }
  C.nsc_index.reset(new uint32_t[n]);
  C.slot.reset(new uint64_t[n]);
  for (size_t i = 0; i < n; ++i) { C.nsc_index[i] = 0; C.slot[i] = 0x5555555555555555ull; }
  return C;
}
