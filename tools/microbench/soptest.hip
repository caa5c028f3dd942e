// soptest.hip — the SOP engine's arithmetic cores on the device, one case per lane, for comparison with exact
// integers (tests/test_sop_arith_gpu.py; the vectors and the checks: tests/sop_vectors.py): the final reduction
// sop_reduce (lcv_sop.hpp), the Montgomery product / square fp_mul_c28 / fp_sqr_c28 and the column products and
// reduction sop_mac28 / sop_kara_mac / sop_kara_join / sop_redc28 (lcv_col28.hpp).  This program only moves data: it
// judges no result.
//
//   soptest IN OUT        (exit status 0: every case ran and OUT is complete)
//
// IN: little-endian uint32 words, three sections in this order, each a count n followed by n fixed-width records:
//   reduce   15 words: r[13] (a value below 2^red p), red (1..15), use_table (0 / 1; 1 only with red <= 3: q p is
//                      read from the LDS table built by sop_qp_entry, else sop_reduce gets nullptr)
//   c28      24 words: a[12], b[12] (values below 2p)
//   columns 377 words: K (1..15), flags (bit 0: Karatsuba, bit 1: 15-limb X, schoolbook only), then 15 slots of
//                      X[13], Y[12] (the operands as the engine forms them, X = m (t0 + t1) on 13 words, below 2^392
//                      unless the 15-limb flag is set; slots >= K are ignored)
// OUT: the results in the same order, no counts:
//   reduce   13 words: r after sop_reduce
//   c28      26 words: fp_mul_c28(a, b)[13], fp_sqr_c28(a)[13]
//   columns  69 words: the 28 column sums after the K products (and the join) as uint64 (low word first), then
//                      sop_redc28 of them [13]
//
// With -DLCV_HOSTSIM (g++, -x c++) only the per-case functions below are compiled: tests/test_sop_arith_cpu.py runs
// the same columns case on the CPU.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../light-client-consensus-specs_amd/csrc \
//         -I../../light-client-consensus-specs_amd/build soptest.hip -o soptest
#include "lcv_sop.hpp"

enum : uint32_t {
  ST_REDUCE_IN = 15, ST_REDUCE_OUT = 13, ST_C28_IN = 24, ST_C28_OUT = 26,
  ST_KMAX = 15, ST_COL_IN = 2 + ST_KMAX * 25, ST_COL_OUT = 56 + 13,
  // q p table entries kept in LDS: sop_reduce reads entry q of a value the host admitted (below 2^(382 + red),
  // so q < 2^(red + 2) <= 32 with the table); those from SOP_QP_N on are zero and reached by no vector in contract
  ST_QP_ENTRIES = 32
};

// the products of one columns record into col (raw column sums), as sop_products does: FIRST on product 0
LCV_FN void soptest_columns(uint64_t col[28], const uint32_t* rec) {
  const uint32_t K = rec[0];
  const bool kara = rec[1] & 1u, x15 = rec[1] & 2u;
  uint64_t p0[13], p2[13];
  int64_t pd[13];
  LCV_NOUNROLL for (uint32_t k = 0; k < K; ++k) {
    const uint32_t* xw = rec + 2 + 25 * k;
    uint32_t Xw[13], Yw[12], X[15], Y[14];
    LCV_UNROLL for (int j = 0; j < 13; ++j) Xw[j] = xw[j];
    LCV_UNROLL for (int j = 0; j < 12; ++j) Yw[j] = xw[13 + j];
    lcv::sop_to28<12, 14>(Y, Yw);
    if (kara) {
      lcv::sop_to28<13, 14>(X, Xw);
      if (k == 0) lcv::sop_kara_mac<true>(p0, p2, pd, X, Y);
      else lcv::sop_kara_mac<false>(p0, p2, pd, X, Y);
    } else if (x15) {
      lcv::sop_to28<13, 15>(X, Xw);
      if (k == 0) lcv::sop_mac28<15, true>(col, X, Y);
      else lcv::sop_mac28<15, false>(col, X, Y);
    } else {
      lcv::sop_to28<13, 14>(X, Xw);
      if (k == 0) lcv::sop_mac28<14, true>(col, X, Y);
      else lcv::sop_mac28<14, false>(col, X, Y);
    }
  }
  if (kara) lcv::sop_kara_join(col, p0, p2, pd);
}

#if !defined(LCV_HOSTSIM)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

__global__ __launch_bounds__(64) void k_reduce(const uint32_t* in, uint32_t n, uint32_t* out) {
  __shared__ __attribute__((aligned(16))) uint32_t qp[16 * ST_QP_ENTRIES];
  if (threadIdx.x < ST_QP_ENTRIES) {
    if (threadIdx.x < lcv::SOP_QP_N) lcv::sop_qp_entry(qp + 16 * threadIdx.x, threadIdx.x);
    else for (int j = 0; j < 16; ++j) qp[16 * threadIdx.x + j] = 0;
  }
  __syncthreads();
  const uint32_t id = blockIdx.x * 64 + threadIdx.x;
  if (id >= n) return;
  const uint32_t* rec = in + (size_t)id * ST_REDUCE_IN;
  uint32_t r[13];
  for (int j = 0; j < 13; ++j) r[j] = rec[j];
  lcv::sop_reduce(r, rec[13], rec[14] ? qp : nullptr);
  for (int j = 0; j < 13; ++j) out[(size_t)id * ST_REDUCE_OUT + j] = r[j];
}

__global__ __launch_bounds__(64) void k_c28(const uint32_t* in, uint32_t n, uint32_t* out) {
  const uint32_t id = blockIdx.x * 64 + threadIdx.x;
  if (id >= n) return;
  const uint32_t* rec = in + (size_t)id * ST_C28_IN;
  uint32_t a[12], b[12], r[13];
  for (int j = 0; j < 12; ++j) { a[j] = rec[j]; b[j] = rec[12 + j]; }
  uint32_t* o = out + (size_t)id * ST_C28_OUT;
  lcv::fp_mul_c28(r, a, b);
  for (int j = 0; j < 13; ++j) o[j] = r[j];
  lcv::fp_sqr_c28(r, a);
  for (int j = 0; j < 13; ++j) o[13 + j] = r[j];
}

__global__ __launch_bounds__(64) void k_columns(const uint32_t* in, uint32_t n, uint32_t* out) {
  const uint32_t id = blockIdx.x * 64 + threadIdx.x;
  if (id >= n) return;
  uint64_t col[28];
  soptest_columns(col, in + (size_t)id * ST_COL_IN);
  uint32_t* o = out + (size_t)id * ST_COL_OUT;
  for (int c = 0; c < 28; ++c) { o[2 * c] = (uint32_t)col[c]; o[2 * c + 1] = (uint32_t)(col[c] >> 32); }
  uint32_t r[13];
  lcv::sop_redc28(r, col);
  for (int j = 0; j < 13; ++j) o[56 + j] = r[j];
}

#define HIP_OK(call)                                                                             \
  do {                                                                                           \
    const hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                      \
      fprintf(stderr, "soptest: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);    \
      return 2;                                                                                  \
    }                                                                                            \
  } while (0)

struct Section { size_t at, n; uint32_t win, wout; };

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: soptest IN OUT\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "soptest: cannot open %s\n", argv[1]); return 2; }
  std::vector<unsigned char> raw;
  {
    unsigned char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    const bool bad = ferror(f) || raw.size() % 4;
    fclose(f);
    if (bad) { fprintf(stderr, "soptest: %s: read error or a size that is no multiple of 4\n", argv[1]); return 2; }
  }
  std::vector<uint32_t> in(raw.size() / 4);
  if (!in.empty()) memcpy(in.data(), raw.data(), raw.size());
  // the three sections: every count against the file size, before anything is launched
  Section sec[3] = {{0, 0, ST_REDUCE_IN, ST_REDUCE_OUT}, {0, 0, ST_C28_IN, ST_C28_OUT}, {0, 0, ST_COL_IN, ST_COL_OUT}};
  size_t at = 0, out_words = 0;
  for (Section& s : sec) {
    if (at >= in.size()) { fprintf(stderr, "soptest: %s ends before a section count\n", argv[1]); return 2; }
    s.n = in[at++];
    if (s.n > (in.size() - at) / s.win) { fprintf(stderr, "soptest: %s is shorter than its counts\n", argv[1]); return 2; }
    s.at = at;
    at += s.n * s.win;
    out_words += s.n * s.wout;
  }
  if (at != in.size()) { fprintf(stderr, "soptest: %s is longer than its counts\n", argv[1]); return 2; }
  // record fields that select code paths or index tables
  for (size_t i = 0; i < sec[0].n; ++i) {
    const uint32_t* r = &in[sec[0].at + i * ST_REDUCE_IN];
    const uint32_t red = r[13], tab = r[14];
    bool ok = red >= 1 && red <= 15 && tab <= 1 && (!tab || red <= 3);
    // the value below 2^(382 + red): word 12 has no bit from 382 + red - 384 up (word 11's top bits when red = 1)
    if (ok) ok = red >= 2 ? (r[12] >> (red - 2)) == 0 : (r[12] == 0 && (r[11] >> 31) == 0);
    if (!ok) { fprintf(stderr, "soptest: reduce record %zu is malformed\n", i); return 2; }
  }
  for (size_t i = 0; i < sec[2].n; ++i) {
    const uint32_t* r = &in[sec[2].at + i * ST_COL_IN];
    if (r[0] < 1 || r[0] > ST_KMAX || r[1] > 2) { fprintf(stderr, "soptest: columns record %zu is malformed\n", i); return 2; }
  }
  uint32_t *din = nullptr, *dout = nullptr;
  HIP_OK(hipMalloc(&din, 4 * in.size()));
  HIP_OK(hipMalloc(&dout, 4 * (out_words + 1)));
  HIP_OK(hipMemcpy(din, in.data(), 4 * in.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dout, 0, 4 * (out_words + 1)));
  size_t oat = 0;
  for (int s = 0; s < 3; ++s) {
    const uint32_t n = (uint32_t)sec[s].n, blocks = (n + 63) / 64;
    if (n) {
      if (s == 0) k_reduce<<<blocks, 64>>>(din + sec[s].at, n, dout + oat);
      if (s == 1) k_c28<<<blocks, 64>>>(din + sec[s].at, n, dout + oat);
      if (s == 2) k_columns<<<blocks, 64>>>(din + sec[s].at, n, dout + oat);
      HIP_OK(hipGetLastError());
    }
    oat += sec[s].n * sec[s].wout;
  }
  HIP_OK(hipDeviceSynchronize());
  std::vector<uint32_t> out(out_words);
  if (out_words) HIP_OK(hipMemcpy(out.data(), dout, 4 * out_words, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(din));
  HIP_OK(hipFree(dout));
  f = fopen(argv[2], "wb");
  if (!f) { fprintf(stderr, "soptest: cannot open %s\n", argv[2]); return 2; }
  const bool wrote = fwrite(out.data(), 4, out_words, f) == out_words;
  if (fclose(f) != 0 || !wrote) { fprintf(stderr, "soptest: %s: write error\n", argv[2]); return 2; }
  printf("soptest: %zu reduce, %zu c28, %zu columns cases\n", sec[0].n, sec[1].n, sec[2].n);
  return 0;
}
#endif
