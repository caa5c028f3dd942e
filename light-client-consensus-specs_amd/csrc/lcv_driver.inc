// lcv_driver.inc — implementation of include/lcv.h over an abstract execution backend.
// Included by lcv_hip.hip (HIP streams / kernels on gfx950: the product, liblcv.so) and by
// lcv_hostsim.cpp (plain host loops: test-only liblcv_hostsim.so).  The including file provides
// `struct Backend`, the LCV_HD qualifier for functor call operators, and the be_* interface that
// lcv_backend.hpp declares.
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lcv.h"
#include "lcv_items.hpp"
#include "lcv_fold.hpp"
#include "lcv_producer.hpp"
#include "lcv_wire_enc.hpp"
#include "lcv_wire_dec.hpp"
#include "lcv_dedup.hpp"
#include "lcv_dedup_plan.hpp"
#include "lcv_sop.hpp"
#include "lcv_rlc.hpp"
#include "lcv_build_id.h"  // LCV_BUILD_ID (Makefile: tools/build_id.py over the sources)

using namespace lcv;

// One mark per kernel launch (marks never nest, so the host simulation's op counter attributes every
// operation to exactly one stage, and a HIP event pair brackets exactly one kernel on its stream).
enum { ST_NSC = 0, ST_PRE, ST_H2C_MAP, ST_H2C, ST_SIG, ST_AGG, ST_MILLER, ST_FEXP, ST_VERDICT, ST_SETUP,
       ST_LINES, ST_LINES_SIG, ST_SIGROOT, ST_RANK, ST_FOLD, ST_PRODUCE_VIEWS, ST_PRODUCE_ROWS, ST_DEDUP,
       ST_RLC_SCALE, ST_RLC_PROD, ST_RLC_SPREAD, ST_RLC_RETRY, ST_WIRE_ENCODE, ST_COUNT };
static const char* kStageNames[ST_COUNT] = {"nsc_htr", "pre_checks", "h2c_sswu", "hash_to_g2", "sig_decode",
                                            "g1_aggregate", "miller_loop", "final_exp", "verdict",
                                            "setup", "miller_lines", "miller_lines_sig", "signing_root",
                                            "store_rank", "store_fold", "produce_views", "produce_rows",
                                            "dedup_gather", "rlc_scale", "rlc_product", "rlc_spread", "rlc_retry",
                                            "wire_encode"};
// lcv_batch_decode's launches: timed like the others, but past the public list (lcv_stage_name, lcv_last_timings);
// lcv_last_decode_timings reports them; likewise lcv_batch_classify's (lcv_last_classify_timings)
enum { ST_WIRE_DECODE = ST_COUNT, ST_DECODE_POOL, ST_CLASS_KEY, ST_CLASS_CONFIRM, ST_TOTAL };

#define LCV_TRY(x)                    \
  do {                                \
    int _rc = (x);                    \
    if (_rc != LCV_OK) return _rc;    \
  } while (0)

// ---- memory.  Every allocation of the driver has one owner, and a new feature allocates through these types only:
//   DevBuf / PinBuf  a device / pinned host buffer that lives in the context (or in a resident batch): pointer and
//                    capacity, grown on demand under the caller's policy, released by lcv_destroy (lcv_batch_free).
//                    No destructor: a release goes through the backend, which lcv_destroy tears down before the
//                    context's members go
//   Scratch          device memory of one call, freed when the call returns, on every path
//   Layout           consecutive 256-byte aligned offsets into one allocation
// be_free waits for every stream, so where a buffer is regrown or a scratch freed is part of a call's schedule
template <bool PINNED> struct Buf {
  uint8_t* p = nullptr;
  size_t cap = 0;  // in the caller's unit
  void release(lcv_ctx* ctx) {
    if (p) PINNED ? be_host_free(ctx, p) : be_free(ctx, p);
    p = nullptr;
    cap = 0;
  }
  // a new buffer of `bytes` for a capacity of new_cap, in place of the old one; empty after a failure
  int renew(lcv_ctx* ctx, size_t new_cap, size_t bytes, bool zero = false) {
    release(ctx);
    void* q = nullptr;
    LCV_TRY(PINNED ? be_host_alloc(ctx, &q, bytes) : be_alloc(ctx, &q, bytes));
    p = (uint8_t*)q;
    cap = new_cap;
    const int rc = zero ? be_memset(ctx, p, 0, bytes) : LCV_OK;
    if (rc != LCV_OK) release(ctx);
    return rc;
  }
  // only grows: the growth policy (new_cap) is the caller's
  int grow(lcv_ctx* ctx, size_t new_cap, size_t bytes) { return (p && new_cap <= cap) ? LCV_OK : renew(ctx, new_cap, bytes); }
  int grow(lcv_ctx* ctx, size_t bytes) { return grow(ctx, bytes, bytes); }
};
typedef Buf<false> DevBuf;
typedef Buf<true> PinBuf;

struct Scratch {
  lcv_ctx* ctx;
  uint8_t* p = nullptr;
  explicit Scratch(lcv_ctx* c) : ctx(c) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { release(); }
  int alloc(size_t bytes) {
    void* q = nullptr;
    LCV_TRY(be_alloc(ctx, &q, bytes));
    p = (uint8_t*)q;
    return LCV_OK;
  }
  void release() {  // (ahead of the return, where the call still has backend work to do behind the free)
    if (p) be_free(ctx, p);
    p = nullptr;
  }
};

struct Layout {
  size_t end = 0;
  size_t take(size_t bytes) {
    const size_t off = end;
    end += (bytes + 255) & ~(size_t)255;
    return off;
  }
  size_t total() const { return end; }
};

struct CommitteeBufs {
  DevBuf raw, pts, sum_all, badmask, key_status;
  size_t ncomm_cap = 0;
  uint32_t ncomm = 0;
  uint32_t raw_stride = 0;
  void release(lcv_ctx* ctx) {
    for (DevBuf* b : {&raw, &pts, &sum_all, &badmask, &key_status}) b->release(ctx);
    ncomm_cap = 0;
    ncomm = raw_stride = 0;
  }
};

struct lcv_dbatch {
  DevBuf mem;
  BatchDev B;
  uint64_t n = 0, npool = 0;
  // a batch that carries its store_index column (B.store_index) is validated against the store table; the
  // column's largest entry is recorded on the host when the column is taken, so that every later validation can
  // check it against the table of that moment in O(1), before any launch
  uint32_t max_store = 0;
  // lcv_set_dedup.  A resident batch uploaded while the mode was on keeps its class column on the host (cls[i]: the
  // first row whose BLS inputs equal row i's; empty: uploaded with the mode off, validated without deduplication), and
  // a table batch also the two columns the committee choice of a row depends on, so that every validation can group
  // the rows under the table of that moment.  lcv_batch_classify makes the same columns for any resident batch, on the
  // device; lcv_batch_fan_out's result inherits them (any labels: equal labels, equal BLS inputs apart from the
  // committee).  A staged host batch brings its grouping along instead (batch_cols
  // COL_DEDUP_REP, COL_DEDUP_UROW; plan_m items, 0: none)
  std::vector<uint32_t> cls, h_store;
  std::vector<uint64_t> h_sig_slot;
  const uint32_t* plan_rep = nullptr;
  const uint32_t* plan_urow = nullptr;
  uint32_t plan_m = 0;
};

// What the pinned `out` region of a HostSlot holds, [n verdicts][n reasons][fold result(s)][status records], by the
// entry that put the batch there: nothing a wait could hand out (lcv_validate_resident_async, a failed enqueue), the two
// arrays alone (lcv_validate_async, _stores_async), with one fold result (_async_fold), with one per store present
// (_stores_async_fold), or a relay's: a status record per message, without or with its fold's per-store results
enum ResultKind : uint8_t { RES_NONE, RES_VERDICTS, RES_FOLD, RES_FOLD_SEG, RES_RELAY, RES_RELAY_FOLD };
struct SlotResults {
  ResultKind kind = RES_NONE;
  size_t n = 0, nseg = 0, nmsg = 0;  // rows; stores present (the by-store kinds); messages (the relay kinds)
  bool by_store() const { return kind == RES_FOLD_SEG || kind == RES_RELAY_FOLD; }
  bool relay() const { return kind == RES_RELAY || kind == RES_RELAY_FOLD; }
};
// ... and where its parts begin, the one place that knows (the two arrays alone keep one result's room behind them: a
// slot that alternates between lcv_validate_async and lcv_validate_async_fold does not regrow)
struct ResultOffsets { size_t reasons, fold, rec, total; };
static ResultOffsets results_offsets(const SlotResults& r) {
  const size_t fold = 2 * r.n;
  const size_t rec = fold + (size_t)FOLD_RESULT_BYTES * (r.by_store() ? r.nseg : r.kind == RES_RELAY ? 0 : 1);
  return {r.n, fold, rec, rec + (size_t)DEC_REC_BYTES * r.nmsg};
}

// host-input serving path (lcv_validate_async and its kin, lcv_relay_async): per work-space slot, a pinned host staging
// copy of what the batch brings (so the host->device copy is a DMA that overlaps the other slots' kernels), its device
// copy, and the pinned region `out` the results are copied back into at the end of the slot's pipeline.  `res` says
// what `out` holds: set last by the entry that enqueued the batch, cleared before a buffer is regrown (stage_transit)
// and by any other asynchronous batch on the slot, read by the waits.  ctx->hsync: the same, synchronous, on slot 0
struct HostSlot {
  PinBuf pinned;
  DevBuf dev;
  PinBuf out;
  SlotResults res;
  std::vector<uint32_t> seg_store;  // the by-store kinds' scatter map: the store row of each of the nseg results
  lcv_dbatch db;  // (a view of `dev`: owns nothing)
  void release(lcv_ctx* ctx) {
    dev.release(ctx);
    pinned.release(ctx);
    out.release(ctx);
  }
};

// the rows of a store-table batch grouped by store (fold_segments): the distinct stores present, ascending; each
// one's rows in ascending order; the present stores' fold states, gathered.  `key` is the grouping's scratch
struct FoldSegs {
  std::vector<uint64_t> key;
  std::vector<uint32_t> store, off, row;
  std::vector<FoldState> in;
  uint32_t nseg = 0;
};

// What a work-space slot owns, beside its streams and events (Backend).  The work space and the scratch buffers are
// allocated by the slot's first call that needs them and only grow (ensure_work, ensure_fold_seg, ensure_dedup,
// ensure_rlc: each states its own policy)
struct Slot {
  DevBuf work;  // (capacity: items; pool_cap: the committee-pool items beside it)
  size_t pool_cap = 0;
  Work W;
  // the per-store results of a segmented fold (lcv_validate_stores_fold), FOLD_RESULT_BYTES per store present
  DevBuf seg;
  // lcv_set_dedup: the items' compact columns and a resident chunk's grouping, the pinned buffer that grouping is
  // copied from, and the rows / items of the slot's last batch (lcv_last_dedup)
  DevBuf dedup;
  DedupDev D = {};
  PinBuf plan_pin;
  uint64_t dd_rows = 0, dd_items = 0;
  // lcv_set_rlc: the scratch, laid out for the slot's work-space capacity, and, for lcv_last_rlc, the groups of the
  // slot's last batch and the slots whose scratch counted that batch's retried rows (bit s: slot s)
  DevBuf rlc;
  RlcDev R = {};
  uint64_t rl_groups = 0;
  uint32_t rl_used = 0;
  HostSlot host;  // lcv_validate_async and its kin
  void release(lcv_ctx* ctx) {  // (all but `host`, which lcv_destroy releases after the context's own buffers)
    for (DevBuf* b : {&work, &seg, &dedup, &rlc}) b->release(ctx);
    plan_pin.release(ctx);
  }
};

// The context.  Its memory: every buffer is a DevBuf or PinBuf member, here or in a Slot (what a work-space slot
// owns, the HostSlot of the host-input entries among it); a call's temporary device memory is a Scratch, offsets into
// one allocation come from a Layout, a resident batch from batch_new, and an entry that may allocate host memory runs
// its body in `guarded`.  A new feature allocates through these only; lcv_destroy releases every owner by name or by
// loop, so a new member is released there or leaks in tools/driver_alloc_check.cpp
struct lcv_ctx {
  Backend be;
  std::string err;
  // store snapshot
  bool store_set = false;
  uint64_t store_fin_slot = 0;
  uint32_t next_known = 0;
  NetConfig cfg = net_config_mainnet();  // lcv_set_config
  CommitteeBufs store;
  CommitteeBufs adhoc;  // committee tables of FastAggregateVerify calls
  // store table (lcv_set_store_table): its committees, decoded and summed like the store's, and the per-store
  // columns (finalized slot, current row, next row or STORE_NEXT_UNKNOWN), one device allocation
  bool table_set = false;
  CommitteeBufs table;
  DevBuf table_mem;  // (capacity: store rows)
  StoreDev table_dev = {nullptr, nullptr, nullptr, 0};
  std::vector<uint8_t> adhoc_src;  // the bytes `adhoc` was built from (reused while calls repeat them)
  // work-space slots: slot 0 serves every synchronous call; slots 0 and 1 alternate under
  // lcv_validate_resident_async (up to LCV_SLOTS batches in flight, each on its own pair of streams)
  Slot slot[LCV_SLOTS];
  Work W;  // the active slot's work space
  FoldSegs segs;  // the grouping of the call in progress (staged before the call returns)
  float stage_ms[ST_TOTAL];
  DevBuf sop_mem;  // device copies of the SOP pairing programs (tools/gen_sop.py)
  SopView sop_lines, sop_acc, sop_fexp, sop_h2c, sop_miller, sop_f12mul;
  // chunk pipeline of validate (lcv_set_pipeline; default 1 x 1 = serial stages): a batch is cut into `pipe_chunks` slices whose
  // stage chains run on `pipe_streams` streams, so the stages of different slices overlap
  int pipe_streams = 1, pipe_chunks = 1;
  size_t chunk = 65536;  // rows per chunk of validate (lcv_debug_set_chunk shrinks it for tests)
  // multi-GPU (lcv_comm_*): one communicator per context, RCCL over xGMI on the device backend
  bool comm_ready = false;
  // a collective that failed (RCCL asynchronous error) or did not complete within comm_timeout_s (a peer
  // rank died or hangs): every collective is refused until lcv_comm_shrink / lcv_comm_abort
  bool comm_failed = false;
  double comm_timeout_s = 60.0;
  int comm_nranks = 1, comm_rank = 0;
  DevBuf comm_buf;  // [per_rank] send slice, then [nranks * per_rank] gathered
  // communication buffers outgrown while a collective may be pending: released only by lcv_destroy, because a
  // free waits for every stream without bound (be_free) and a collective call must never block unbounded
  std::vector<DevBuf> comm_retired;
  HostSlot hsync;  // lcv_validate_updates' staging (one pinned buffer, one device copy, reused)
  // no per-stage timing marks (HIP event pairs) while set: the asynchronous entries never collect them,
  // so a serving loop would otherwise grow the event pool without bound
  bool marks_off = false;
  // latency mode (lcv_set_latency_mode): batches of at most fan_max rows run the SOP programs on the fan
  // engine (an op's K products on K lanes, its tail on a 16-lane row, one item per block, lcv_sop_fan.hpp,
  // lcv_sop_row.hpp; both Miller walks and the
  // accumulation as one program) and the SSWU maps / signature decoding on their one-item-per-wave twins
  // (square-root chains spread over the wave, lcv_wave.hpp): one update 6.0 ms on the batch engine -> 2.8 ms
  // (DESIGN.md §3.5).  On by default for the reference's call shape (one update per call)
  uint64_t fan_max = LCV_FAN_MAX_DEFAULT;
  // engine log (lcv_debug_engine_log): launches per engine since the last reset — [0] fan-engine SOP programs,
  // [1] batch-engine SOP programs, [2] one-item-per-wave twins, [3] one-lane-per-item SSWU / signature kernels —
  // and the items per wave of each SOP program's last batch-engine launch (lines, miller_acc, fexp, h2c), so
  // tests can assert which engine a call ran on
  uint64_t eng_count[4] = {0, 0, 0, 0};
  uint32_t eng_items[4] = {0, 0, 0, 0};
  // items per wave of the SOP kernels (k_sop: lines, miller_acc, fexp, h2c); 0 = 64 / team.  Experiment
  // knobs, set from the environment at lcv_init (LCV_SOP_ITEMS_LINES / _ACC / _FEXP / _H2C): fewer items
  // per wave = more waves per SIMD for the same batch (DESIGN §7)
  uint32_t sop_items[4] = {0, 0, 0, 0};
  // deduplicated BLS half (lcv_set_dedup, off by default; include/lcv.h "Deduplicated signatures"; per slot: Slot).
  // dd_*: the host's scratch of the call in progress.  tab_*: the store table's columns as the device holds them, for
  // the host's committee choice (dedup_comm_rows)
  bool dedup = false;
  uint32_t dedup_hash_bits = 64;  // lcv_debug_dedup_hash_bits
  DedupTable dd_table;
  std::vector<uint32_t> dd_cls, dd_comm, dd_rep, dd_urow;
  std::vector<uint64_t> tab_fin;
  std::vector<uint32_t> tab_cur, tab_next;
  // randomised batch verification (lcv_set_rlc, off by default; include/lcv.h "Batch verification"): the group size
  // (0: off) and the seed; the batch counter the next chunk's coefficients are derived from (never reused: +1 per
  // chunk that runs the mode); per slot: Slot
  uint32_t rlc_group = 0;
  bool rlc_seeded = false;
  uint32_t rlc_seed[8] = {};
  uint64_t rlc_counter = 0;
  // lcv_batch_encode's scratch (one chunk of message areas, their result records, the chunk's row list): grown on
  // demand up to LCV_ENCODE_SCRATCH_BYTES of areas, kept for the next call; enc_chunk: lcv_debug_set_encode_chunk
  DevBuf enc_mem;
  uint64_t enc_chunk = 0;
  // lcv_batch_decode's staging: the pinned buffer the messages are copied into and the device scratch one DMA moves
  // them to (followed there by the rows' records and the pool resolution's lists), both grown on demand and kept;
  // dec_hash_bits: lcv_debug_decode_hash_bits; dec_table: the grouping's scratch
  PinBuf dec_pin;
  DevBuf dec_mem;
  uint32_t dec_hash_bits = 64;
  DedupTable dec_table;
  // lcv_relay_async under lcv_set_dedup, the host's scratch of the call in progress: the messages' class tuples
  // (wire_dedup_tuples) and classes, the pairs' signature slots (the pairs' classes, committee rows and items: dd_*)
  std::vector<uint8_t> rl_beacon, rl_bits, rl_sig;
  std::vector<uint64_t> rl_slot, rl_pslot;
  std::vector<uint32_t> rl_cls;
};

static uint32_t host_be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

static int fail(lcv_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

static const size_t kChunk = 65536;  // the largest chunk of validate, and of every entry that takes one chunk per call

// A stage: one mark around its launches (marks never nest, see ST_*).  A launch that fails returns its code with
// the mark left open: nothing collects the timings of a failed call.  bench.py's per-kernel roofline reads the
// marks by name, so every marked launch goes through here
template <class L> static int stage(lcv_ctx* ctx, int st, L&& launch) {
  be_stage_begin(ctx, st);
  LCV_TRY(launch());
  be_stage_end(ctx, st);
  return LCV_OK;
}

// The boundary: the body of an extern "C" entry that may allocate host memory (std::vector, std::string) runs in here,
// so that no exception leaves the library; slot 0 is the active one again after one
static int fail_nothrow(lcv_ctx* ctx, int code, const char* who, const char* what) noexcept {
  try {
    if (ctx) be_set_slot(ctx, 0);
    return fail(ctx, code, std::string(who) + ": " + what);
  } catch (...) {
    return code;
  }
}
template <class Body> static int guarded(lcv_ctx* ctx, const char* who, Body&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail_nothrow(ctx, LCV_ENOMEM, who, "out of host memory");
  } catch (const std::exception& e) {
    return fail_nothrow(ctx, LCV_EINVAL, who, e.what());
  } catch (...) {
    return fail_nothrow(ctx, LCV_EINVAL, who, "unknown exception");
  }
}

#include "lcv_functors_sop.hpp"
#if defined(LCV_CPU_FAST)
#include "lcv_cpu_direct.hpp"
struct F_sig_direct { BatchDev B; Work W; LCV_HD void operator()(uint32_t i) const { item_sig_direct(i, B, W); } };
struct F_h2c_direct { Work W; LCV_HD void operator()(uint32_t i) const { item_h2c_direct(i, W); } };
struct F_pair_direct { Work W; LCV_HD void operator()(uint32_t i) const { item_pairing_direct(i, W); } };
#endif

// The way of every host-input batch into the HostSlot h: `stage_bytes` filled by fill(pinned region) go through h's
// reused pinned staging buffer and ONE DMA into h's reused device copy of dev_bytes, on the slot's main stream, instead
// of a device allocation, one copy per part and a free per call.  slot >= 0 (the enqueuing entries, h =
// ctx->slot[slot].host): the staging buffer is reused only after the slot's previous batch has left it (EV_H2D, recorded
// behind the copy); the slot is waited for before a buffer it may still use is regrown; h.res is cleared BEFORE anything
// regrows (a failed grow leaves an empty buffer; from here on the slot's last batch is this one); slot 0 is the active
// one again on return.  slot < 0: the synchronous entries, h = ctx->hsync, on slot 0; out_bytes 0 (chunk_results' to grow)
template <class Fill>
static int stage_transit(lcv_ctx* ctx, int slot, HostSlot& h, size_t stage_bytes, size_t dev_bytes, size_t out_bytes,
                         Fill&& fill) {
  const bool async = slot >= 0;
  be_set_slot(ctx, async ? slot : 0);
  int rc = async ? be_wait_event(ctx, EV_H2D) : LCV_OK;
  if (async && rc == LCV_OK && (stage_bytes > h.pinned.cap || dev_bytes > h.dev.cap || out_bytes > h.out.cap))
    rc = be_sync_slot(ctx);
  h.res = SlotResults{};
  if (rc == LCV_OK) rc = h.pinned.grow(ctx, stage_bytes);
  if (rc == LCV_OK && out_bytes) rc = h.out.grow(ctx, out_bytes);
  if (rc == LCV_OK) rc = h.dev.grow(ctx, dev_bytes);
  if (rc == LCV_OK) {
    fill(h.pinned.p);
    be_set_slot(ctx, async ? slot : 0);  // (be_free above may not keep the slot)
    rc = be_h2d(ctx, h.dev.p, h.pinned.p, stage_bytes);
    if (async && rc == LCV_OK) rc = be_mark(ctx, EV_H2D, 0);
  }
  if (async) be_set_slot(ctx, 0);
  return rc;
}

// ------------------------------------------------------------------ helpers
// latency mode for batches of at most ctx->fan_max rows: the fan engine for the SOP programs (identical results,
// lcv_sop_fan.hpp) and the one-item-per-wave twins of the SSWU maps and the signature decoding (launch_items)
static bool fan_on(const lcv_ctx* ctx, uint64_t rows) { return rows > 0 && rows <= ctx->fan_max; }
// one-lane-per-item kernels: latency-mode batches take the inlined twins of the SSWU maps and the signature
// decoding (lcv_k_lat.hip), identical results
template <class F> static int launch_items(lcv_ctx* ctx, const F& f, uint32_t n, uint64_t rows) {
  const bool twin = fan_on(ctx, rows);
  ctx->eng_count[twin ? 2 : 3] += 1;
  if constexpr (std::is_same<F, F_h2c_map>::value) {
    if (twin) return be_launch(ctx, F_h2c_map_lat{f.W}, n);
  }
  if constexpr (std::is_same<F, F_sig>::value) {
    if (twin) return be_launch(ctx, F_sig_lat{f.B, f.W}, n);
  }
  return be_launch(ctx, f, n);
}
// index of a batch-engine SOP program in ctx->sop_items / eng_items (the fused Miller program is fan-only)
template <class F> static constexpr int sop_prog_index() {
  return std::is_same<F, F_sop_lines>::value ? 0 : std::is_same<F, F_sop_acc>::value ? 1
       : std::is_same<F, F_sop_fexp>::value ? 2 : std::is_same<F, F_sop_h2c>::value ? 3 : -1;
}
// SOP programs: the fan engine for latency-mode batches, the batch engine otherwise (identical results).
// Batch engine: g items per one-wave block, the most that fit (64 / TEAM) unless LCV_SOP_ITEMS_<PROGRAM>
// (read at lcv_init) asks for fewer
template <class F> static int launch_sop(lcv_ctx* ctx, const F& f, uint32_t n, uint64_t rows) {
  if (fan_on(ctx, rows)) {
    ctx->eng_count[0] += 1;
    return be_launch_sop_fan(ctx, f, n);
  }
  constexpr int k = sop_prog_index<F>();
  static_assert(k >= 0, "launch_sop: a batch-engine program");
  constexpr uint32_t G = 64 / F::TEAM;
  uint32_t g = ctx->sop_items[k];
  if (g == 0 || g > G) g = G;
  ctx->eng_count[1] += 1;
  ctx->eng_items[k] = g;
  return be_launch_sop(ctx, f, n, g);
}

// ---- the work space and the deduplication scratch, each described once: one row per array of a Work (lcv_items.hpp)
// and of a DedupDev (lcv_dedup.hpp), in allocation order — the pointer member, the element size, the elements per
// item (`rows`) and the kind, which names the kernels' own index function.  Allocation (ensure_work, ensure_dedup),
// slicing (work_view) and the layout check (lcv_debug_work_check) are derived from these rows and those functions;
// nothing else states a stride.  A new array is a new member and a new row here
enum FieldKind { FK_SOA, FK_F, FK_LINES, FK_POOL, FK_RANK, FK_SPACE, FK_ITEM };  // (field_index)
struct Field { const char* name; size_t slot, esize, rows; FieldKind kind; };
#define LCV_FIELD(T, m, rows, kind) {#m, offsetof(T, m), sizeof(*T().m), rows, kind}
static constexpr Field kWorkFields[] = {
    LCV_FIELD(Work, msg, 8, FK_SOA),           LCV_FIELD(Work, pre_reason, 1, FK_SOA),
    LCV_FIELD(Work, comm_id, 1, FK_SOA),       LCV_FIELD(Work, nsc_eq, 1, FK_SOA),
    LCV_FIELD(Work, nsc_root, 8, FK_POOL),     LCV_FIELD(Work, nsc_flags, 1, FK_POOL),
    LCV_FIELD(Work, qmap, 96, FK_SOA),         LCV_FIELD(Work, qh, 48, FK_SOA),
    LCV_FIELD(Work, qh_inf, 1, FK_SOA),        LCV_FIELD(Work, qs, 48, FK_SOA),
    LCV_FIELD(Work, sig_status, 1, FK_SOA),    LCV_FIELD(Work, pk, 24, FK_SOA),
    LCV_FIELD(Work, agg_status, 1, FK_SOA),    LCV_FIELD(Work, f, F12_ITEM_WORDS, FK_F),
    LCV_FIELD(Work, pair_ok, 1, FK_SOA),       LCV_FIELD(Work, verdict, 1, FK_SOA),
    LCV_FIELD(Work, reason, 1, FK_SOA),        LCV_FIELD(Work, lines, SOP_LINE_WORDS, FK_LINES),
    LCV_FIELD(Work, rank, RANK_BYTES, FK_RANK), LCV_FIELD(Work, fold_out, FOLD_RESULT_BYTES, FK_SPACE),
};
static constexpr Field kDedupFields[] = {
    LCV_FIELD(DedupDev, att_beacon, K_BEACON, FK_ITEM), LCV_FIELD(DedupDev, sig_slot, 1, FK_ITEM),
    LCV_FIELD(DedupDev, bits, K_BITS, FK_ITEM),         LCV_FIELD(DedupDev, sig, K_SIG, FK_ITEM),
    LCV_FIELD(DedupDev, comm_id, 1, FK_ITEM),           LCV_FIELD(DedupDev, rep, 1, FK_ITEM),
    LCV_FIELD(DedupDev, urow, 1, FK_ITEM),
};
// the batch-verification scratch (lcv_rlc.hpp RlcDev), laid out for the slot's work-space capacity
static constexpr Field kRlcFields[] = {
    LCV_FIELD(RlcDev, pk_s, 24, FK_SOA),              LCV_FIELD(RlcDev, g1_s, 24, FK_SOA),
    LCV_FIELD(RlcDev, prod_a, F12_ITEM_WORDS, FK_F),  LCV_FIELD(RlcDev, prod_b, F12_ITEM_WORDS, FK_F),
    LCV_FIELD(RlcDev, g_ok, 1, FK_SOA),               LCV_FIELD(RlcDev, retry, 1, FK_SOA),
    LCV_FIELD(RlcDev, cnt, 4, FK_SPACE),
};
static_assert(sizeof(RlcDev) == sizeof(kRlcFields) / sizeof(Field) * sizeof(void*), "an RlcDev array without a row in kRlcFields");
// every pointer member has its row (a Work also holds cap and pool_cap in one pointer-sized word, msg_b0 in another)
static_assert(sizeof(Work) == (2 + sizeof(kWorkFields) / sizeof(Field)) * sizeof(void*), "a Work array without a row in kWorkFields");
static_assert(sizeof(DedupDev) == sizeof(kDedupFields) / sizeof(Field) * sizeof(void*), "a DedupDev array without a row in kDedupFields");

// a pointer member of a device struct by its offset (every table here names members that way)
static uint8_t* slot_get(const void* obj, size_t slot) {
  uint8_t* p;
  memcpy(&p, (const uint8_t*)obj + slot, sizeof(p));
  return p;
}
static void slot_set(void* obj, size_t slot, const void* p) { memcpy((uint8_t*)obj + slot, &p, sizeof(p)); }

// element r of item i of a field, in elements, as the kernels address it
static size_t field_index(const Field& f, size_t cap, size_t pool_cap, size_t i, size_t r) {
  switch (f.kind) {
    case FK_SOA: return soa_index(cap, i, r);  // stride cap
    case FK_F: return f12_index(i, (uint32_t)(r / 12)) + r % 12;
    case FK_LINES: return lines_index(i) + r;
    case FK_POOL: return soa_index(pool_cap, i, r);  // one item per distinct committee, not per update
    case FK_RANK: return rank_index(i) + r;
    case FK_SPACE: return r;              // one per work space (the fold's result): a single item
    case FK_ITEM: return i * f.rows + r;  // item-major rows (the deduplication scratch, never sliced)
  }
  return 0;
}
static bool field_per_item(const Field& f) { return f.kind != FK_POOL && f.kind != FK_SPACE; }
static size_t field_items(const Field& f, size_t cap, size_t pool_cap) {
  return f.kind == FK_POOL ? pool_cap : f.kind == FK_SPACE ? 1 : cap;
}
// the arrays of `o` (null: the sizes only), each at the next 256-byte aligned offset of m and as long as its last
// item's last element reaches; returns the bytes taken
template <size_t N> static size_t fields_bind(void* o, const Field (&tab)[N], uint8_t* m, size_t cap, size_t pool_cap) {
  Layout l;
  for (const Field& f : tab) {
    const size_t off = l.take(f.esize * (field_index(f, cap, pool_cap, field_items(f, cap, pool_cap) - 1, f.rows - 1) + 1));
    if (o) slot_set(o, f.slot, m + off);
  }
  return l.total();
}

// the work space of `slot` (allocated or grown on demand; be_free waits for the streams) becomes ctx->W.  Neither
// capacity ever shrinks; at least 64 items and a pool of 1; zero-filled
static int ensure_work(lcv_ctx* ctx, size_t cap, size_t pool_cap, int slot = 0) {
  Slot& s = ctx->slot[slot];
  if (!s.work.p || cap > s.work.cap || pool_cap > s.pool_cap) {
    cap = std::max({cap, s.work.cap, (size_t)64});
    pool_cap = std::max({pool_cap, s.pool_cap, (size_t)1});
    LCV_TRY(s.work.renew(ctx, cap, fields_bind(nullptr, kWorkFields, nullptr, cap, pool_cap), true));
    s.pool_cap = pool_cap;
    s.W = Work{};
    s.W.cap = (uint32_t)cap;
    s.W.pool_cap = (uint32_t)pool_cap;
    fields_bind(&s.W, kWorkFields, s.work.p, cap, pool_cap);
  }
  ctx->W = s.W;
  return LCV_OK;
}

// the deduplication scratch of `slot` for chunks of up to `cap` rows (lcv_set_dedup): 284 bytes per item (the four
// compact batch columns and the compact committee ids) and 8 per row (a resident chunk's rep / urow), as large as the
// slot's work space at least; allocated by the slot's first deduplicated call (be_free waits for the streams)
static int ensure_dedup(lcv_ctx* ctx, size_t cap, int slot) {
  Slot& s = ctx->slot[slot];
  cap = std::max(cap, s.work.cap);
  if (s.dedup.p && cap <= s.dedup.cap) return LCV_OK;
  LCV_TRY(s.dedup.renew(ctx, cap, fields_bind(nullptr, kDedupFields, nullptr, cap, 0)));
  fields_bind(&s.D, kDedupFields, s.dedup.p, cap, 0);
  return LCV_OK;
}
// the batch-verification scratch of `slot` (lcv_set_rlc), laid out for the slot's work-space capacity of this moment
// (pk_s stands in for W.pk, with W's stride), so it follows the work space when that grows; zero-filled; allocated by
// the slot's first call with the mode on (be_free waits for the streams)
static int ensure_rlc(lcv_ctx* ctx, int slot) {
  Slot& s = ctx->slot[slot];
  const size_t cap = s.work.cap;
  if (s.rlc.p && cap == s.rlc.cap) return LCV_OK;
  LCV_TRY(s.rlc.renew(ctx, cap, fields_bind(nullptr, kRlcFields, nullptr, cap, 0), true));
  fields_bind(&s.R, kRlcFields, s.rlc.p, cap, 0);
  return LCV_OK;
}
// the BLS stages' view of a deduplicated chunk of m items: the compact columns where they read the batch's and W's
static void dedup_batch_view(const DedupDev& D, uint32_t m, BatchDev& Bu, Work& Wu) {
  Bu.att_beacon = D.att_beacon; Bu.sig_slot = D.sig_slot; Bu.bits = D.bits; Bu.sig = D.sig; Bu.n = m;
  Wu.comm_id = D.comm_id;
}

// the five arrays of ncomm committees, all or none: a failed allocation leaves `cb` empty
static int ensure_committees(lcv_ctx* ctx, CommitteeBufs& cb, size_t ncomm, uint32_t raw_stride) {
  if (ncomm > cb.ncomm_cap || raw_stride != cb.raw_stride || !cb.raw.p) {
    cb.release(ctx);
    int rc = cb.raw.renew(ctx, ncomm, ncomm * raw_stride);
    if (rc == LCV_OK) rc = cb.pts.renew(ctx, ncomm, ncomm * 512 * 24 * 4);
    if (rc == LCV_OK) rc = cb.sum_all.renew(ctx, ncomm, ncomm * 36 * 4);
    if (rc == LCV_OK) rc = cb.badmask.renew(ctx, ncomm, ncomm * 16 * 4);
    if (rc == LCV_OK) rc = cb.key_status.renew(ctx, ncomm, ncomm * 512);
    if (rc != LCV_OK) {
      cb.release(ctx);
      return rc;
    }
    cb.ncomm_cap = ncomm;
    cb.raw_stride = raw_stride;
  }
  cb.ncomm = (uint32_t)ncomm;
  return LCV_OK;
}

static CommitteeDev committee_view(const CommitteeBufs& cb, const uint8_t* next_raw) {
  CommitteeDev C;
  C.next_raw = next_raw;
  C.pts = (uint32_t*)cb.pts.p;
  C.sum_all = (uint32_t*)cb.sum_all.p;
  C.badmask = (uint32_t*)cb.badmask.p;
  C.key_status = cb.key_status.p;
  C.raw = cb.raw.p;
  C.raw_stride = cb.raw_stride;
  C.ncomm = cb.ncomm;
  return C;
}

// decode + KeyValidate every key, then per-committee sums / invalid-key masks
static int build_committees(lcv_ctx* ctx, CommitteeBufs& cb) {
  CommitteeDev C = committee_view(cb, nullptr);
  return stage(ctx, ST_SETUP, [&] {
    LCV_TRY(be_launch(ctx, F_key{C}, cb.ncomm * 512));
    return be_launch_team(ctx, F_sum{C}, cb.ncomm);
  });
}

#define LCV_SOP_SRC(name) {kSop_##name##_hdr, sizeof(kSop_##name##_hdr)}, \
    {kSop_##name##_rec, sizeof(kSop_##name##_rec)}, {kSop_##name##_consts, sizeof(kSop_##name##_consts)}
static int upload_sop(lcv_ctx* ctx) {
  struct Src { const void* p; size_t bytes; };
  enum { NSRC = 18 };
  const Src src[NSRC] = {LCV_SOP_SRC(lines), LCV_SOP_SRC(miller_acc), LCV_SOP_SRC(fexp), LCV_SOP_SRC(h2c),
                         LCV_SOP_SRC(miller), LCV_SOP_SRC(f12mul)};
  size_t off[NSRC];
  Layout l;
  for (int k = 0; k < NSRC; ++k) off[k] = l.take(src[k].bytes);
  LCV_TRY(ctx->sop_mem.grow(ctx, l.total()));
  uint8_t* m = ctx->sop_mem.p;
  for (int k = 0; k < NSRC; ++k) LCV_TRY(be_h2d(ctx, m + off[k], src[k].p, src[k].bytes));
  auto view = [&](int k, uint32_t rounds, uint32_t slots, uint32_t nconst) {
    return SopView{(const uint32_t*)(m + off[3 * k]), (const uint32_t*)(m + off[3 * k + 1]),
                   (const uint32_t*)(m + off[3 * k + 2]), rounds, slots, nconst};
  };
  ctx->sop_lines = view(0, LCV_SOP_LINES_ROUNDS, LCV_SOP_LINES_SLOTS, LCV_SOP_LINES_NCONST);
  ctx->sop_acc = view(1, LCV_SOP_MILLER_ACC_ROUNDS, LCV_SOP_MILLER_ACC_SLOTS, LCV_SOP_MILLER_ACC_NCONST);
  ctx->sop_fexp = view(2, LCV_SOP_FEXP_ROUNDS, LCV_SOP_FEXP_SLOTS, LCV_SOP_FEXP_NCONST);
  ctx->sop_h2c = view(3, LCV_SOP_H2C_ROUNDS, LCV_SOP_H2C_SLOTS, LCV_SOP_H2C_NCONST);
  ctx->sop_miller = view(4, LCV_SOP_MILLER_ROUNDS, LCV_SOP_MILLER_SLOTS, LCV_SOP_MILLER_NCONST);
  ctx->sop_f12mul = view(5, LCV_SOP_F12MUL_ROUNDS, LCV_SOP_F12MUL_SLOTS, LCV_SOP_F12MUL_NCONST);
  return be_sync(ctx);
}

// items [base, base + n) of the work space: the same layout with every per-item array advanced to its item
// `base`, which is right because each kind's index function is additive in the item (lcv_debug_work_check (1));
// the committee-pool arrays and the fold's result are not per item
static Work work_view(const Work& W, size_t base) {
  Work v = W;
  for (const Field& f : kWorkFields)
    if (field_per_item(f)) slot_set(&v, f.slot, slot_get(&W, f.slot) + f.esize * field_index(f, W.cap, W.pool_cap, base, 0));
  return v;
}

// The end of every pairing check, written once: the Miller value of items [0, n) — the accumulation over both
// pairings' lines in W.lines, or (fused; latency mode) both walks and the accumulation as one fan-engine program
// (F_sop_miller; the signature's G2 subgroup check happens inside: W.sig_status) — then the final exponentiation
static bool fused_miller(const lcv_ctx* ctx, uint64_t rows) { return fan_on(ctx, rows); }
static int miller_fexp(lcv_ctx* ctx, const Work& W, uint32_t n, bool fused) {
  LCV_TRY(stage(ctx, ST_MILLER, [&] {
    if (!fused) return launch_sop(ctx, F_sop_acc{W, ctx->sop_acc}, n, n);
    ctx->eng_count[0] += 1;
    return be_launch_sop_fan(ctx, F_sop_miller{W, ctx->sop_miller}, n);
  }));
  return stage(ctx, ST_FEXP, [&] { return launch_sop(ctx, F_sop_fexp{W, ctx->sop_fexp}, n, n); });
}

// pairing check of W.qh / W.qs / W.pk for items [0, n), on one stream (lcv_debug_pairing): the SOP programs
// (lcv_functors_sop.hpp) — the lines of both pairings in one launch (2n teams), then miller_fexp
static int pairing_check(lcv_ctx* ctx, const Work& W, uint32_t n) {
  if (fused_miller(ctx, n)) return miller_fexp(ctx, W, n, true);
  LCV_TRY(stage(ctx, ST_LINES, [&] { return launch_sop(ctx, F_sop_lines{W, ctx->sop_lines, 0u}, 2 * n, n); }));
  return miller_fexp(ctx, W, n, false);
}

// hash_to_G2 of W.msg for items [0, n) -> W.qh, W.qh_inf: two SSWU lanes per update, then the
// team program (isogeny, addition, cofactor clearing, affine)
static int hash_to_g2_stage(lcv_ctx* ctx, const Work& W, uint32_t n) {
  LCV_TRY(launch_items(ctx, F_h2c_map{W}, 2 * n, n));
  return launch_sop(ctx, F_sop_h2c{W, ctx->sop_h2c}, n, n);
}

// signature decode (one lane per update), then the signature pairing's line walk, which ends with the
// G2 subgroup check of the signature (psi(Q) == [x]Q) -> W.qs, W.sig_status (and that pairing's lines)
static int sig_decode_check(lcv_ctx* ctx, const BatchDev& B, const Work& W, uint32_t n) {
  LCV_TRY(launch_items(ctx, F_sig{B, W}, n, n));
  return launch_sop(ctx, F_sop_lines{W, ctx->sop_lines, 1u}, n, n);
}

// masked aggregation of the participants' keys (team kernel; agg_items > n: slices folded into item 0)
static int agg_stage(lcv_ctx* ctx, const BatchDev& B, const CommitteeDev& C, const Work& W, uint32_t n,
                     uint32_t agg_items) {
  return stage(ctx, ST_AGG, [&] {
    if (agg_items <= n) return be_launch_team(ctx, F_agg_team{B, C, W}, n);
    LCV_TRY(be_launch_team(ctx, F_agg_team{B, C, W}, agg_items));
    return be_launch(ctx, F_agg_fold{W, agg_items}, 1);
  });
}

// the non-BLS asserts of items [0, n): against the context's store, or (S: a batch with a store_index) each update
// against its own row of the store table — the per-update committee equality (item_nsc_eq_team) then runs ahead
// of the table form of item_pre on the same stream
static int pre_stage(lcv_ctx* ctx, const BatchDev& B, const CommitteeDev& C, const Params& P, const StoreDev* S,
                     const Work& W, uint32_t n) {
  if (!S) return be_launch(ctx, F_pre{B, C, P, W}, n);
  LCV_TRY(be_launch_team(ctx, F_nsc_eq_team{B, C, *S, P, W}, n));
  return be_launch(ctx, F_pre_table{B, *S, P, W}, n);
}

// the rank records of items [0, n) (the _fold calls, lcv_rank_*)
static int rank_stage(lcv_ctx* ctx, const BatchDev& B, const Params& P, const Work& W, uint32_t n) {
  return stage(ctx, ST_RANK, [&] { return be_launch(ctx, F_rank{B, P, W}, n); });
}

#if defined(LCV_CPU_FAST)
// run_bls of the CPU-baseline build: direct per-update code (lcv_cpu_direct.hpp), one core per update, in
// program order (never deduplicated: dedup_on)
static int run_bls_direct(lcv_ctx* ctx, const BatchDev& B, const CommitteeDev& C, uint32_t n, uint32_t agg_items,
                          const Params* P, const BatchDev* nsc, const StoreDev* S, bool rank) {
  const Work& W = ctx->W;
  if (nsc) LCV_TRY(be_launch_team(ctx, F_nsc_team{*nsc, C, W}, nsc->npool));
  if (P) {
    LCV_TRY(pre_stage(ctx, B, C, *P, S, W, n));
    if (rank) LCV_TRY(rank_stage(ctx, B, *P, W, n));
    LCV_TRY(be_launch(ctx, F_sigroot{B, *P, W}, n));
  }
  LCV_TRY(stage(ctx, ST_SIG, [&] { return be_launch(ctx, F_sig_direct{B, W}, n); }));
  LCV_TRY(stage(ctx, ST_H2C, [&] { return be_launch(ctx, F_h2c_direct{W}, n); }));
  LCV_TRY(stage(ctx, ST_AGG, [&] {
    LCV_TRY(be_launch(ctx, F_agg{B, C, W}, agg_items > n ? agg_items : n));
    return agg_items > n ? be_launch(ctx, F_agg_fold{W, agg_items}, 1) : LCV_OK;
  }));
  LCV_TRY(stage(ctx, ST_MILLER, [&] { return be_launch(ctx, F_pair_direct{W}, n); }));
  return stage(ctx, ST_VERDICT, [&] { return be_launch(ctx, F_verdict{W}, n); });
}
#endif

// A deduplicated chunk of validate (lcv_set_dedup): the grouping of its n rows into m items (rep, urow: device
// pointers) is known, D is the slot's scratch for the items' compact columns
struct DedupRun { DedupDev D; const uint32_t* rep; const uint32_t* urow; uint32_t m; };

// A chunk of validate under randomised batch verification (lcv_set_rlc): groups of `group` = 1 << shift consecutive
// items, the coefficients' key (seed, this chunk's batch counter), D the slot's scratch
struct RlcRun { RlcDev D; RlcKey key; uint32_t shift; };

// a batch-engine launch of the mode's own SOP functors (never on the fan engine: the mode acts on batch-engine chunks
// only), counted in the engine log like launch_sop's; `prog`: the program's index in ctx->sop_items, or -1
template <class F> static int launch_sop_rlc(lcv_ctx* ctx, const F& f, uint32_t n, int prog) {
  constexpr uint32_t G = 64 / F::TEAM;
  uint32_t g = prog >= 0 ? ctx->sop_items[prog] : 0;
  if (g == 0 || g > G) g = G;
  ctx->eng_count[1] += 1;
  if (prog >= 0) ctx->eng_items[prog] = g;
  return be_launch_sop(ctx, f, n, g);
}

// The end of the pairing check of a batch-verified chunk, after the Miller accumulation (W.f: the items' scaled Miller
// values), on the main stream: the product tree over each group (shift launches with halving item counts, ping-pong
// between the scratch's two arrays), the unchanged final exponentiation over the groups (a Work view: f -> the
// products, pair_ok -> g_ok), the spread of the groups' results, and the unchanged final exponentiation again over the
// items of failing groups, whose number stays on the device (worst-case grid)
static int rlc_finish(lcv_ctx* ctx, const Work& W, uint32_t m, uint32_t flags, const RlcRun& L) {
  const RlcDev& D = L.D;
  const uint32_t* src = W.f;
  uint32_t src_n = m;
  LCV_TRY(stage(ctx, ST_RLC_PROD, [&]() -> int {
    for (uint32_t level = 0; level < L.shift; ++level) {
      uint32_t* dst = (level & 1u) ? D.prod_b : D.prod_a;
      const uint32_t n = (src_n + 1) / 2;
      LCV_TRY(launch_sop_rlc(ctx, F_sop_f12mul{W, ctx->sop_f12mul, src, dst, src_n, level, flags}, n, -1));
      src = dst;
      src_n = n;
    }
    return LCV_OK;
  }));
  Work Wg = W;
  Wg.f = const_cast<uint32_t*>(src);
  Wg.pair_ok = D.g_ok;
  LCV_TRY(stage(ctx, ST_FEXP, [&] { return launch_sop(ctx, F_sop_fexp{Wg, ctx->sop_fexp}, src_n, m); }));
  LCV_TRY(stage(ctx, ST_RLC_SPREAD, [&] { return be_launch(ctx, F_rlc_spread{W, D, L.shift, flags}, m); }));
  return stage(ctx, ST_RLC_RETRY, [&] {
    constexpr uint32_t G = 64 / F_sop_fexp_rows::TEAM;
    uint32_t g = ctx->sop_items[2];
    if (g == 0 || g > G) g = G;
    ctx->eng_count[1] += 1;
    return be_launch_sop_counted(ctx, F_sop_fexp_rows{W, ctx->sop_fexp, D.retry}, D.cnt, m, g);
  });
}

// The BLS half of the pipeline for rows [0, n) on two streams of the active slot (a main stream and a
// side stream), ordered by events:
//   side: [HTR(next_sync_committee)] [item_pre: reasons, committee ids] [rank records], signature decode, [masked
//         aggregation, without committee hashing] -> EV_PRE, (after EV_H2C) the signature pairing's line
//         walk with the fused G2 subgroup check -> EV_SIDE
//   main: [signing root] SSWU maps, hash_to_G2 tail, (after EV_PRE) [masked aggregation, with committee
//         hashing] -> EV_H2C, the message pairing's line walk, (after EV_SIDE) Miller accumulation, final
//         exponentiation, verdict
// hash_to_G2 (1,250 one-wave blocks per 10^4 updates) is round-latency bound: a line walk beside it took
// 4.3 ms instead of 2.25, so both walks run side by side after it (profiles/r02_v7: 693k -> 719k
// updates/s).  P (validate) adds item_pre and the signing root; nsc (first chunk) adds the committee
// roots; FastAggregateVerify passes neither (its W.msg / W.comm_id are set by the caller).
// agg_items > n (FastAggregateVerify of > 512 keys, n == 1): the aggregation runs over agg_items
// slices and item_agg_fold sums them into item 0.  S: the store table of a batch with a store_index (pre_stage).
// rank (the _fold calls only): the rank records of the slice (F_rank) follow the pre-checks on the side stream.
//
// R (a deduplicated chunk; with P): the pre-checks and the rank records run over the n rows as ever, then
//   side: F_dedup_gather -> EV_GATHER, and the main stream's work waits for EV_GATHER
// and from there every BLS stage runs over the R->m items — m sizes every launch and picks the engine — on the
// items' compact columns (Bu) and compact committee ids (Wu.comm_id), which the gather takes from what item_pre
// wrote; F_verdict_dedup then gives each of the n rows its item's verdict.  Without R the items are the rows.
static int run_bls(lcv_ctx* ctx, const BatchDev& B, const CommitteeDev& C, uint32_t n, uint32_t agg_items = 0,
                   const Params* P = nullptr, const BatchDev* nsc = nullptr, const StoreDev* S = nullptr,
                   bool rank = false, const DedupRun* R = nullptr, const RlcRun* L = nullptr) {
  const Work& W = ctx->W;
#if defined(LCV_CPU_FAST)
  if (!W.msg_b0) return run_bls_direct(ctx, B, C, n, agg_items, P, nsc, S, rank);
#endif
  const uint32_t m = R ? R->m : n;
  BatchDev Bu = B;
  Work Wu = W;
  if (R) dedup_batch_view(R->D, m, Bu, Wu);
  if (L && fan_on(ctx, m)) L = nullptr;  // the mode acts on batch-engine chunks only
  // the message pairing's walk reads the scaled aggregate key where it reads W.pk
  Work Ws = Wu;
  if (L) Ws.pk = L->D.pk_s;
  auto scale = [&] { return stage(ctx, ST_RLC_SCALE, [&] { return be_launch(ctx, F_rlc_scale{Wu, L->key, L->D}, m); }); };
  LCV_TRY(be_mark(ctx, EV_START, 0));
  LCV_TRY(be_wait(ctx, 1, EV_START));  // the side stream starts after the slot's earlier main-stream work
  be_use_stream(ctx, 1);
  if (nsc) LCV_TRY(stage(ctx, ST_NSC, [&] { return be_launch_team(ctx, F_nsc_team{*nsc, C, W}, nsc->npool); }));
  if (P) {
    LCV_TRY(stage(ctx, ST_PRE, [&] { return pre_stage(ctx, B, C, *P, S, W, n); }));
    if (rank) LCV_TRY(rank_stage(ctx, B, *P, W, n));
  }
  if (R) {
    LCV_TRY(stage(ctx, ST_DEDUP, [&] { return be_launch_team(ctx, F_dedup_gather{B, W, R->urow, R->D}, m); }));
    LCV_TRY(be_mark(ctx, EV_GATHER, 1));
  }
  LCV_TRY(stage(ctx, ST_SIG, [&] { return launch_items(ctx, F_sig{Bu, Wu}, m, m); }));
  // the masked aggregation needs item_pre's committee ids only.  It runs here, off the main stream's
  // SSWU -> hash_to_G2 chain, the longer one (one update: 2.4 ms against 2.2 on this stream with the
  // committee hashed) — unless the slice hashes a large pool of distinct committees (configs[3]: one per
  // update), which makes this stream the longer one: then it stays on the main stream, after EV_PRE
  const bool agg_side = nsc == nullptr || nsc->npool < 64;
  if (agg_side) LCV_TRY(agg_stage(ctx, Bu, C, Wu, m, agg_items));
  if (agg_side && L) LCV_TRY(scale());
  LCV_TRY(be_mark(ctx, EV_PRE, 1));
  be_use_stream(ctx, 0);
  if (R) LCV_TRY(be_wait(ctx, 0, EV_GATHER));
  if (P) LCV_TRY(stage(ctx, ST_SIGROOT, [&] { return be_launch(ctx, F_sigroot{Bu, *P, Wu}, m); }));
  LCV_TRY(stage(ctx, ST_H2C_MAP, [&] { return launch_items(ctx, F_h2c_map{Wu}, 2 * m, m); }));
  LCV_TRY(stage(ctx, ST_H2C, [&] { return launch_sop(ctx, F_sop_h2c{Wu, ctx->sop_h2c}, m, m); }));
  // item_pre's ids and (agg_side) the aggregate key, before EV_H2C: the message pairing's walk then follows
  // hash_to_G2 in stream order, with no wait of its own, and is dispatched ahead of the signature's walk
  // (which waits on EV_H2C) — with both behind cross-stream waits they share the CUs evenly and the Miller
  // accumulation after them measured 1.75 -> 1.9-2.3 ms per 10^4 batch (profiles/r05_v3/serial_ab.txt)
  LCV_TRY(be_wait(ctx, 0, EV_PRE));
  if (!agg_side) LCV_TRY(agg_stage(ctx, Bu, C, Wu, m, agg_items));
  if (!agg_side && L) LCV_TRY(scale());  // before EV_H2C, which the signature's walk waits for
  const bool fused = fused_miller(ctx, m);  // latency mode: EV_PRE (after the side stream's last kernel) joins it
  if (!fused) {
    LCV_TRY(be_mark(ctx, EV_H2C, 0));
    be_use_stream(ctx, 1);
    LCV_TRY(be_wait(ctx, 1, EV_H2C));
    LCV_TRY(stage(ctx, ST_LINES_SIG, [&] {
      if (L) return launch_sop_rlc(ctx, F_sop_lines_g1{Wu, ctx->sop_lines, L->D.g1_s}, m, 0);
      return launch_sop(ctx, F_sop_lines{Wu, ctx->sop_lines, 1u}, m, m);
    }));
    LCV_TRY(be_mark(ctx, EV_SIDE, 1));
    be_use_stream(ctx, 0);
    LCV_TRY(stage(ctx, ST_LINES, [&] { return launch_sop(ctx, F_sop_lines{Ws, ctx->sop_lines, 2u}, m, m); }));
    LCV_TRY(be_wait(ctx, 0, EV_SIDE));
  }
  if (L) {
    // excluded from its group: an item whose verdict does not read pair_ok; the rows' pre-checks count where the
    // items are the rows
    LCV_TRY(stage(ctx, ST_MILLER, [&] { return launch_sop(ctx, F_sop_acc{Wu, ctx->sop_acc}, m, m); }));
    LCV_TRY(rlc_finish(ctx, Wu, m, (P && !R) ? RLC_PRE : 0u, *L));
  } else {
    LCV_TRY(miller_fexp(ctx, Wu, m, fused));
  }
  return stage(ctx, ST_VERDICT, [&] {
    return R ? be_launch(ctx, F_verdict_dedup{W, R->rep}, n) : be_launch(ctx, F_verdict{W}, n);
  });
}

// The whole per-update chain (pre-checks, signature decode + subgroup check, hash_to_G2, masked
// aggregation, Miller loop, final exponentiation, verdict) for one slice, on the current stream.
// Slices are independent, so the sliced pipeline of validate runs slice k on stream k % pipe_streams: the
// kernels of different slices overlap, filling the CUs that one stage's tail (or a one-lane-per-update stage)
// leaves idle.  No stage marks of its own: concurrent kernels would inflate each other's event times.  S: the
// store table of a batch that carries its store_index (pre_stage).
static int run_slice(lcv_ctx* ctx, const BatchDev& B, const CommitteeDev& C, const Params& P, const StoreDev* S,
                     const Work& W, uint32_t n, bool rank = false) {
  LCV_TRY(pre_stage(ctx, B, C, P, S, W, n));
  if (rank) LCV_TRY(be_launch(ctx, F_rank{B, P, W}, n));  // the _fold calls: this slice's rank records
  LCV_TRY(be_launch(ctx, F_sigroot{B, P, W}, n));
  LCV_TRY(sig_decode_check(ctx, B, W, n));
  LCV_TRY(hash_to_g2_stage(ctx, W, n));
  LCV_TRY(be_launch_team(ctx, F_agg_team{B, C, W}, n));
  LCV_TRY(launch_sop(ctx, F_sop_lines{W, ctx->sop_lines, 2u}, n, n));
  LCV_TRY(miller_fexp(ctx, W, n, false));
  return be_launch(ctx, F_verdict{W}, n);
}

// ------------------------------------------------------------------ API
extern "C" {

const char* lcv_last_error(const lcv_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

const char* lcv_stage_name(int stage) { return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : "?"; }

int lcv_init(int device, lcv_ctx** out) {
  if (!out) return LCV_EINVAL;
  *out = nullptr;
  lcv_ctx* ctx = new (std::nothrow) lcv_ctx();
  if (!ctx) return LCV_ENOMEM;
  int rc = be_init(ctx, device);
  if (rc != LCV_OK) {
    delete ctx;
    return rc;
  }
  for (int s = 0; s < ST_TOTAL; ++s) ctx->stage_ms[s] = 0.f;
  {
    const char* names[4] = {"LCV_SOP_ITEMS_LINES", "LCV_SOP_ITEMS_ACC", "LCV_SOP_ITEMS_FEXP", "LCV_SOP_ITEMS_H2C"};
    for (int k = 0; k < 4; ++k)
      if (const char* e = getenv(names[k])) ctx->sop_items[k] = (uint32_t)atoi(e);
  }
  rc = upload_sop(ctx);
  if (rc != LCV_OK) {
    lcv_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return LCV_OK;
}

void lcv_destroy(lcv_ctx* ctx) {
  if (!ctx) return;
  // every owner, before the backend goes
  ctx->table_mem.release(ctx);
  for (CommitteeBufs* cb : {&ctx->store, &ctx->adhoc, &ctx->table}) cb->release(ctx);
  for (Slot& s : ctx->slot) s.release(ctx);
  for (DevBuf* b : {&ctx->sop_mem, &ctx->enc_mem, &ctx->dec_mem}) b->release(ctx);
  ctx->dec_pin.release(ctx);
  ctx->comm_buf.release(ctx);
  for (DevBuf& b : ctx->comm_retired) b.release(ctx);
  for (Slot& s : ctx->slot) s.host.release(ctx);
  ctx->hsync.release(ctx);
  if (ctx->comm_ready) be_comm_destroy(ctx);
  be_destroy(ctx);
  delete ctx;
}

int lcv_set_store(lcv_ctx* ctx, uint64_t finalized_slot, const uint8_t* cur, const uint8_t* next, uint8_t* key_status_out) {
  if (!ctx || !cur || !next) return fail(ctx, LCV_EINVAL, "lcv_set_store: null argument");
  LCV_TRY(ensure_committees(ctx, ctx->store, 2, K_SC));
  LCV_TRY(be_h2d(ctx, ctx->store.raw.p, cur, K_SC));
  LCV_TRY(be_h2d(ctx, ctx->store.raw.p + K_SC, next, K_SC));
  be_reset_timings(ctx);
  LCV_TRY(build_committees(ctx, ctx->store));
  if (key_status_out) LCV_TRY(be_d2h(ctx, key_status_out, ctx->store.key_status.p, 1024));
  LCV_TRY(be_sync(ctx));
  uint32_t any = 0;
  for (int k = 0; k < K_SC; ++k) any |= next[k];
  ctx->next_known = any ? 1u : 0u;  // is_next_sync_committee_known (sync-protocol.md:316-317)
  ctx->store_fin_slot = finalized_slot;
  ctx->store_set = true;
  return LCV_OK;
}

}  // extern "C"

// The columns of a packed batch, each at a 256-byte aligned offset of one device allocation: the 13 of
// lcv_update_batch, which every batch has, then the optional ones, empty where unused, which so travel with the
// batch in its one copy — the per-update store-table rows of lcv_validate_updates_stores; the grouping of the rows
// by store and the present stores' fold states of a segmented fold (lcv_validate_stores_fold; FoldSegs: store,
// off, row, in); the grouping of a staged batch's rows into BLS items under lcv_set_dedup (DedupCols: rep, urow)
enum BatchCol {
  COL_ATT_BEACON = 0, COL_ATT_EXEC, COL_ATT_BRANCH, COL_FIN_BEACON, COL_FIN_EXEC, COL_FIN_BRANCH, COL_NSC_POOL,
  COL_NSC_INDEX, COL_NSC_BRANCH, COL_FINALITY_BRANCH, COL_BITS, COL_SIG, COL_SIG_SLOT,
  COL_STORE_INDEX, COL_SEG_STORE, COL_SEG_OFF, COL_SEG_ROW, COL_SEG_IN, COL_DEDUP_REP, COL_DEDUP_UROW,
  BATCH_COLS, BATCH_COLS_REQUIRED = COL_STORE_INDEX
};
struct DedupCols { const uint32_t* rep; const uint32_t* urow; uint32_t m; };
struct BatchCols {
  const void* src[BATCH_COLS];
  size_t bytes[BATCH_COLS], off[BATCH_COLS];
  size_t total = 0, n = 0, np = 0;
};
// One row per BatchCol, in the enum's order: the bytes of an element; what counts the elements; the member of BatchDev
// it is bound to, with the same member of ProdOut (the producer's writable view of the row columns); the member of
// lcv_update_batch it is read from or written to (download); -1 where there is none.  Layout, sources, binding,
// slicing and the copies out are derived from these rows: a new column is a new enum entry and a new row here
// (ColCount, in batch_layout's order: n; np; n with a store_index; ng; ng + 1 and n in a segmented fold; n in a batch
// staged with its grouping into BLS items; nd)
enum ColCount { CN_ROWS, CN_POOL, CN_ROWS_IF_STORES, CN_SEGS, CN_SEGS_1, CN_ROWS_IF_SEGS, CN_ROWS_IF_ITEMS, CN_ITEMS };
struct ColSpec { size_t width; ColCount count; int dev, prod, host; };
#define LCV_COL_ROW(w, dev, host) {w, CN_ROWS, (int)offsetof(BatchDev, dev), (int)offsetof(ProdOut, dev), (int)offsetof(lcv_update_batch, host)}
static constexpr ColSpec kBatchCols[] = {
    LCV_COL_ROW(K_BEACON, att_beacon, attested.beacon),
    LCV_COL_ROW(K_EXEC, att_exec, attested.execution),
    LCV_COL_ROW(K_EXEC_BRANCH, att_branch, attested.exec_branch),
    LCV_COL_ROW(K_BEACON, fin_beacon, finalized.beacon),
    LCV_COL_ROW(K_EXEC, fin_exec, finalized.execution),
    LCV_COL_ROW(K_EXEC_BRANCH, fin_branch, finalized.exec_branch),
    {K_SC, CN_POOL, (int)offsetof(BatchDev, nsc_pool), -1, (int)offsetof(lcv_update_batch, nsc_pool)},
    LCV_COL_ROW(sizeof(uint32_t), nsc_index, nsc_index),
    LCV_COL_ROW(K_NSC_BRANCH, nsc_branch, nsc_branch),
    LCV_COL_ROW(K_FIN_BRANCH, finality_branch, finality_branch),
    LCV_COL_ROW(K_BITS, bits, sync_bits),
    LCV_COL_ROW(K_SIG, sig, sync_signature),
    LCV_COL_ROW(sizeof(uint64_t), sig_slot, signature_slot),
    {sizeof(uint32_t), CN_ROWS_IF_STORES, (int)offsetof(BatchDev, store_index), -1, -1},
    {sizeof(uint32_t), CN_SEGS, -1, -1, -1},          // COL_SEG_STORE
    {sizeof(uint32_t), CN_SEGS_1, -1, -1, -1},        // COL_SEG_OFF
    {sizeof(uint32_t), CN_ROWS_IF_SEGS, -1, -1, -1},  // COL_SEG_ROW
    {sizeof(FoldState), CN_SEGS, -1, -1, -1},         // COL_SEG_IN
    {sizeof(uint32_t), CN_ROWS_IF_ITEMS, -1, -1, -1}, // COL_DEDUP_REP
    {sizeof(uint32_t), CN_ITEMS, -1, -1, -1},         // COL_DEDUP_UROW
};
static_assert(sizeof(kBatchCols) / sizeof(ColSpec) == BATCH_COLS, "one row per BatchCol");
// the columns a slice advances (chunk_view) and a download copies row by row: the per-row members of BatchDev
static bool col_per_row(const ColSpec& s) { return s.dev >= 0 && s.count != CN_POOL; }

// the layout alone (no host sources): n rows, np pool rows, with a store_index column or not, ng fold segments,
// nd BLS items (0: no grouping)
static void batch_layout(BatchCols& c, size_t n, size_t np, bool stores, size_t ng, size_t nd = 0) {
  const size_t count[] = {n, np, stores ? n : 0, ng, ng ? ng + 1 : 0, ng ? n : 0, nd ? n : 0, nd};  // by ColCount
  Layout l;
  for (int k = 0; k < BATCH_COLS; ++k) {
    c.src[k] = nullptr;
    c.bytes[k] = kBatchCols[k].width * count[kBatchCols[k].count];
    c.off[k] = l.take(c.bytes[k]);
  }
  c.total = l.total();
  c.n = n;
  c.np = np;
}

static int batch_cols(lcv_ctx* ctx, const lcv_update_batch* hb, BatchCols& c, const char* who,
                      const uint32_t* store_index = nullptr, const FoldSegs* segs = nullptr,
                      const DedupCols* dd = nullptr) {
  const size_t n = hb->n, np = hb->npool, ng = segs ? segs->nseg : 0;
  if (n == 0 || np == 0 || n > 0xffffffffull || np > 0xffffffffull)
    return fail(ctx, LCV_EINVAL, std::string(who) + ": need 0 < n, 0 < npool < 2^32");
  const void* src[BATCH_COLS] = {};
  for (int k = 0; k < BATCH_COLS; ++k)
    if (kBatchCols[k].host >= 0) src[k] = slot_get(hb, kBatchCols[k].host);
  src[COL_STORE_INDEX] = store_index;
  if (ng) {
    src[COL_SEG_STORE] = segs->store.data(); src[COL_SEG_OFF] = segs->off.data();
    src[COL_SEG_ROW] = segs->row.data(); src[COL_SEG_IN] = segs->in.data();
  }
  if (dd) { src[COL_DEDUP_REP] = dd->rep; src[COL_DEDUP_UROW] = dd->urow; }
  for (int k = 0; k < BATCH_COLS_REQUIRED; ++k)
    if (!src[k]) return fail(ctx, LCV_EINVAL, std::string(who) + ": null column");
  batch_layout(c, n, np, store_index != nullptr, ng, dd ? dd->m : 0);
  for (int k = 0; k < BATCH_COLS; ++k) c.src[k] = src[k];
  for (size_t i = 0; i < n; ++i)
    if (hb->nsc_index[i] >= np) return fail(ctx, LCV_EINVAL, std::string(who) + ": nsc_index out of range");
  return LCV_OK;
}

// db's column pointers into device memory m laid out as c
static void bind_batch(lcv_dbatch* db, uint8_t* m, const BatchCols& c) {
  auto at = [&](BatchCol k) { return m + c.off[k]; };
  BatchDev& B = db->B;
  for (int k = 0; k < BATCH_COLS; ++k)  // an optional column that the batch does not carry is null
    if (kBatchCols[k].dev >= 0)
      slot_set(&B, kBatchCols[k].dev, k < BATCH_COLS_REQUIRED || c.bytes[k] ? at((BatchCol)k) : nullptr);
  B.n = (uint32_t)c.n;
  B.npool = (uint32_t)c.np;
  db->n = c.n;
  db->npool = c.np;
  db->max_store = 0;
  if (c.bytes[COL_STORE_INDEX]) {
    const uint32_t* ix = (const uint32_t*)c.src[COL_STORE_INDEX];
    for (size_t i = 0; i < c.n; ++i)
      if (ix[i] > db->max_store) db->max_store = ix[i];
  }
  // a staged batch's grouping into BLS items (lcv_set_dedup), where it was staged
  const bool plan = c.bytes[COL_DEDUP_UROW] != 0;
  db->plan_rep = plan ? (const uint32_t*)at(COL_DEDUP_REP) : nullptr;
  db->plan_urow = plan ? (const uint32_t*)at(COL_DEDUP_UROW) : nullptr;
  db->plan_m = (uint32_t)(c.bytes[COL_DEDUP_UROW] / 4);
}

// ---- deduplicated BLS half, host side (lcv_set_dedup; lcv_dedup_plan.hpp).  The CPU-baseline build's direct branch
// of run_bls runs every row, so there the mode groups nothing (lcv_last_dedup: items == rows)
#if defined(LCV_CPU_FAST)
static bool dedup_on(const lcv_ctx*) { return false; }
#else
static bool dedup_on(const lcv_ctx* ctx) { return ctx->dedup; }
#endif
// comm[i] = the committee-table row the signature of row i is checked against, as item_pre_table chooses it under
// the store table that is set (every store_index has been checked against it)
static void dedup_comm_rows(const lcv_ctx* ctx, const uint32_t* store_index, const uint64_t* sig_slot, size_t n, uint32_t* comm) {
  for (size_t i = 0; i < n; ++i) {
    const uint32_t s = store_index[i], cur = ctx->tab_cur[s];
    comm[i] = sig_committee_row(period_of_slot(sig_slot[i], ctx->cfg), period_of_slot(ctx->tab_fin[s], ctx->cfg), cur,
                                table_next_row(cur, ctx->tab_next[s]));
  }
}
// the grouping of a one-chunk host batch about to be staged: classes, then items by (class, committee row), into
// the context's scratch; `dd` then names the two columns that travel with the batch.  Off (dd.m == 0) while the mode
// is, and for a batch batch_cols is about to refuse.  Allocates host memory: within the boundary (guarded)
static int dedup_stage(lcv_ctx* ctx, const lcv_update_batch* hb, const uint32_t* store_index, DedupCols& dd) {
  dd = DedupCols{nullptr, nullptr, 0};
  if (!dedup_on(ctx) || hb->n == 0 || hb->n > ctx->chunk || !hb->attested.beacon || !hb->signature_slot || !hb->sync_bits ||
      !hb->sync_signature)
    return LCV_OK;
  const uint32_t n = (uint32_t)hb->n;
  ctx->dd_cls.resize(n);
  ctx->dd_rep.resize(n);
  ctx->dd_urow.resize(n);
  if (store_index) ctx->dd_comm.resize(n);
  dedup_classes(hb->attested.beacon, hb->signature_slot, hb->sync_bits, hb->sync_signature, n, ctx->dedup_hash_bits,
                ctx->dd_cls.data(), ctx->dd_table);
  if (store_index) dedup_comm_rows(ctx, store_index, hb->signature_slot, n, ctx->dd_comm.data());
  dd.m = dedup_plan(ctx->dd_cls.data(), store_index ? ctx->dd_comm.data() : nullptr, n, ctx->dedup_hash_bits,
                    ctx->dd_rep.data(), ctx->dd_urow.data(), ctx->dd_table);
  dd.rep = ctx->dd_rep.data();
  dd.urow = ctx->dd_urow.data();
  return LCV_OK;
}
// the grouping of rows [base, base + n) of a batch for this validation, and the slot's scratch: a staged batch
// brought it along; a resident batch's chunk is grouped here from the columns it keeps on the host, under the table
// of this call, and the two columns go to the device through the slot's pinned buffer in one small copy each
static int dedup_chunk(lcv_ctx* ctx, const lcv_dbatch* db, int slot, size_t base, uint32_t n, DedupRun& R) {
  LCV_TRY(ensure_dedup(ctx, n, slot));
  be_set_slot(ctx, slot);
  Slot& s = ctx->slot[slot];
  R.D = s.D;
  if (db->plan_m) {
    R.rep = db->plan_rep;
    R.urow = db->plan_urow;
    R.m = db->plan_m;
    return LCV_OK;
  }
  LCV_TRY(be_wait_event(ctx, EV_PLAN));  // the slot's previous grouping has left the pinned buffer
  LCV_TRY(s.plan_pin.grow(ctx, 8 * (size_t)n));
  uint32_t* rep = (uint32_t*)s.plan_pin.p;
  uint32_t* urow = rep + n;
  const bool table = !db->h_store.empty();
  if (table) {
    ctx->dd_comm.resize(n);
    dedup_comm_rows(ctx, db->h_store.data() + base, db->h_sig_slot.data() + base, n, ctx->dd_comm.data());
  }
  R.m = dedup_plan(db->cls.data() + base, table ? ctx->dd_comm.data() : nullptr, n, ctx->dedup_hash_bits, rep, urow,
                   ctx->dd_table);
  LCV_TRY(be_h2d(ctx, R.D.rep, rep, 4 * (size_t)n));
  LCV_TRY(be_h2d(ctx, R.D.urow, urow, 4 * (size_t)R.m));
  LCV_TRY(be_mark(ctx, EV_PLAN, 0));
  R.rep = R.D.rep;
  R.urow = R.D.urow;
  return LCV_OK;
}

extern "C" {

void lcv_batch_free(lcv_ctx* ctx, lcv_dbatch* b) {
  if (!ctx || !b) return;
  b->mem.release(ctx);
  delete b;
}

// A resident batch in the making: batch_new allocates it for the layout c and binds its columns; it is abandoned
// (freed) when the call returns, on every path, unless it has been handed out
struct NewBatch {
  lcv_ctx* ctx;
  lcv_dbatch* db = nullptr;
  explicit NewBatch(lcv_ctx* c) : ctx(c) {}
  NewBatch(const NewBatch&) = delete;
  NewBatch& operator=(const NewBatch&) = delete;
  ~NewBatch() { lcv_batch_free(ctx, db); }
  int hand_out(lcv_dbatch** out) {
    *out = db;
    db = nullptr;
    return LCV_OK;
  }
};
static int batch_new(lcv_ctx* ctx, const BatchCols& c, NewBatch& nb) {
  nb.db = new (std::nothrow) lcv_dbatch();
  if (!nb.db) return fail(ctx, LCV_ENOMEM, "resident batch: out of host memory");
  LCV_TRY(nb.db->mem.grow(ctx, c.total));
  bind_batch(nb.db, nb.db->mem.p, c);
  return LCV_OK;
}

static int batch_upload(lcv_ctx* ctx, const lcv_update_batch* hb, const uint32_t* store_index, lcv_dbatch** out) {
  if (!ctx || !hb || !out) return fail(ctx, LCV_EINVAL, "lcv_batch_upload: null argument");
  *out = nullptr;
  return guarded(ctx, "lcv_batch_upload", [&]() -> int {
    BatchCols c;
    LCV_TRY(batch_cols(ctx, hb, c, "lcv_batch_upload", store_index));
    NewBatch nb(ctx);
    LCV_TRY(batch_new(ctx, c, nb));
    lcv_dbatch* db = nb.db;
    if (dedup_on(ctx)) {  // the class column, and what a table batch's committee choice reads, stay on the host
      db->cls.resize(c.n);
      dedup_classes(hb->attested.beacon, hb->signature_slot, hb->sync_bits, hb->sync_signature, (uint32_t)c.n,
                    ctx->dedup_hash_bits, db->cls.data(), ctx->dd_table);
      if (store_index) {
        db->h_store.assign(store_index, store_index + c.n);
        db->h_sig_slot.assign(hb->signature_slot, hb->signature_slot + c.n);
      }
    }
    for (int k = 0; k < BATCH_COLS; ++k) LCV_TRY(be_h2d(ctx, db->mem.p + c.off[k], c.src[k], c.bytes[k]));
    LCV_TRY(be_sync(ctx));
    return nb.hand_out(out);
  });
}

int lcv_batch_upload(lcv_ctx* ctx, const lcv_update_batch* hb, lcv_dbatch** out) {
  return batch_upload(ctx, hb, nullptr, out);
}

// a resident batch that carries its store_index column: every resident entry validates it against the store
// table of the moment of the call (validate_prepare checks the recorded largest index against that table)
int lcv_batch_upload_stores(lcv_ctx* ctx, const lcv_update_batch* hb, const uint32_t* store_index, lcv_dbatch** out) {
  if (!store_index) return fail(ctx, LCV_EINVAL, "lcv_batch_upload_stores: null argument");
  return batch_upload(ctx, hb, store_index, out);
}

int lcv_batch_shape(lcv_ctx* ctx, const lcv_dbatch* b, uint64_t* n_out, uint64_t* npool_out) {
  if (!ctx || !b || !n_out || !npool_out) return fail(ctx, LCV_EINVAL, "lcv_batch_shape: null argument");
  *n_out = b->n;
  *npool_out = b->npool;
  return LCV_OK;
}

// rows [base, base + n) of a batch: every per-row column it carries advanced by `base` elements, the pool as it is
static BatchDev chunk_view(const BatchDev& B, size_t base, uint32_t n) {
  BatchDev c = B;
  for (const ColSpec& s : kBatchCols)
    if (col_per_row(s))
      if (const uint8_t* p = slot_get(&B, s.dev)) slot_set(&c, s.dev, p + s.width * base);
  c.n = n;
  return c;
}

// a fold request of the _fold entries: the state going in and (synchronous form) where the result goes
// segs (lcv_validate_stores_fold): a segmented fold of a store-table batch — `in` is unused, `out` is indexed by
// store row, and seg_dev points at the grouping's columns in the batch's device copy (seg_bind)
struct FoldReq { FoldState in; lcv_fold_result* out; const FoldSegs* segs = nullptr; FoldSegDev seg_dev = {}; };
static_assert(sizeof(lcv_fold_state) == sizeof(FoldState) && sizeof(lcv_fold_result) == sizeof(FoldResult) &&
              sizeof(FoldResult) <= FOLD_RESULT_BYTES, "lcv.h's fold structs are lcv_fold.hpp's");
static int fold_state_in(lcv_ctx* ctx, const char* who, const lcv_fold_state* in, FoldState& s) {
  if (!in) return fail(ctx, LCV_EINVAL, std::string(who) + ": null fold state");
  if (in->previous_max_active_participants > LCV_SYNC_COMMITTEE_SIZE || in->current_max_active_participants > LCV_SYNC_COMMITTEE_SIZE)
    return fail(ctx, LCV_EINVAL, std::string(who) + ": max_active_participants above SYNC_COMMITTEE_SIZE");
  memcpy(&s, in, sizeof(s));
  return LCV_OK;
}
// F_fold over the first n rows of the active work space, on the current stream (after F_verdict in stream order)
static int fold_stage(lcv_ctx* ctx, const FoldState& in, uint64_t store_fin_slot, uint32_t next_known, uint32_t n) {
  return stage(ctx, ST_FOLD, [&] { return be_launch_team(ctx, F_fold{ctx->W, in, store_fin_slot, next_known, n}, 1); });
}
// the segmented fold's device side.  seg_bind: the grouping's four columns in a staged device copy m, at its layout's
// offsets (a host batch's COL_SEG_*, a relay's RelayLayout).  ensure_fold_seg: the slot's result buffer (be_free waits
// for the streams).  fold_seg_stage: F_fold_seg, one team per store present, where fold_stage would run F_fold
static void seg_bind(FoldReq& f, const uint8_t* m, size_t store, size_t off, size_t row, size_t in) {
  f.seg_dev.seg_store = (const uint32_t*)(m + store);
  f.seg_dev.seg_off = (const uint32_t*)(m + off);
  f.seg_dev.seg_row = (const uint32_t*)(m + row);
  f.seg_dev.in = m + in;
}
static int ensure_fold_seg(lcv_ctx* ctx, int slot, size_t nseg) {
  DevBuf& seg = ctx->slot[slot].seg;
  if (seg.p && nseg <= seg.cap) return LCV_OK;
  const size_t cap = std::max({nseg, 2 * seg.cap, (size_t)64});  // doubles
  return seg.renew(ctx, cap, cap * FOLD_RESULT_BYTES);
}
static int fold_seg_stage(lcv_ctx* ctx, const Work& W, const StoreDev& S, const FoldSegDev& G, uint32_t nseg) {
  return stage(ctx, ST_FOLD, [&] { return be_launch_team(ctx, F_fold_seg{W, S, G}, nseg); });
}
// the results of a segmented fold, as they arrived (FOLD_RESULT_BYTES per store present), to the caller's array indexed
// by store row: only the present stores' entries are written
static void fold_seg_scatter(lcv_fold_result* out, const uint8_t* res, const uint32_t* seg_store, size_t nseg) {
  for (size_t g = 0; g < nseg; ++g) memcpy(&out[seg_store[g]], res + FOLD_RESULT_BYTES * g, sizeof(FoldResult));
}

// The results named by r on their way into the pinned region `out`, on the current slot's stream, behind the batch:
// the verdicts and reasons of the work space W, the fold result from W.fold_out or (the by-store kinds) the slot's
// `seg` buffer, a relay's status records from `rec`.  No wait: results_hand_out follows the caller's sync
static int results_enqueue(lcv_ctx* ctx, uint8_t* out, const SlotResults& r, const Work& W, const uint8_t* seg,
                           const uint8_t* rec) {
  const ResultOffsets o = results_offsets(r);
  LCV_TRY(be_d2h(ctx, out, W.verdict, r.n));
  LCV_TRY(be_d2h(ctx, out + o.reasons, W.reason, r.n));
  if (r.by_store()) LCV_TRY(be_d2h(ctx, out + o.fold, seg, (size_t)FOLD_RESULT_BYTES * r.nseg));
  else if (r.kind == RES_FOLD) LCV_TRY(be_d2h(ctx, out + o.fold, W.fold_out, sizeof(FoldResult)));
  if (r.relay()) LCV_TRY(be_d2h(ctx, out + o.rec, rec, (size_t)DEC_REC_BYTES * r.nmsg));
  return LCV_OK;
}
// ... and out of it once they have arrived: the first n verdicts and reasons, the fold result (fold_out indexed by
// store row for the by-store kinds, seg_store their scatter map) and a relay's status bytes, each where the caller
// asks for it and r has it.  Nothing is consumed: a repeated wait hands out the same bytes
static void results_hand_out(const uint8_t* out, const SlotResults& r, const uint32_t* seg_store, size_t n,
                             uint8_t* verdict_out, uint8_t* reason_out, lcv_fold_result* fold_out, uint8_t* status_out) {
  const ResultOffsets o = results_offsets(r);
  if (n && verdict_out) memcpy(verdict_out, out, n);
  if (n && reason_out) memcpy(reason_out, out + o.reasons, n);
  if (fold_out && r.by_store()) fold_seg_scatter(fold_out, out + o.fold, seg_store, r.nseg);
  else if (fold_out && r.kind == RES_FOLD) memcpy(fold_out, out + o.fold, sizeof(FoldResult));
  if (status_out && r.relay())
    for (size_t j = 0; j < r.nmsg; ++j) {
      uint32_t st;
      memcpy(&st, out + o.rec + DEC_REC_BYTES * j, 4);
      status_out[j] = st ? 1 : 0;
    }
}

// What a validation is asked for: where the verdicts and reasons go — to host memory, to a device buffer, or
// (neither) nowhere: they stay in the slot's work space — how it runs, and the fold behind it, if any
struct ValidateReq {
  uint8_t* verdict_host = nullptr;
  uint8_t* reason_host = nullptr;
  uint8_t* verdict_dev = nullptr;
  int slot = -1;  // -1: synchronous, on slot 0 (and more for several chunks); 0..7: enqueued on that slot's streams, no wait
  const FoldReq* fold = nullptr;
};
// ... and what validate_prepare settles for the schedule that serves it
struct ValidateRun {
  lcv_ctx* ctx;
  lcv_dbatch* db;
  ValidateReq q;
  bool async;       // q.slot >= 0
  int slot;         // the work-space slot of a one-chunk batch; its rows and items are counted there (lcv_last_dedup)
  size_t n, cap;    // rows; rows per chunk
  Params P;
  CommitteeDev C;
  const StoreDev* S;       // the store table of a batch that carries its store_index, else null
  const FoldSegs* segs;    // a segmented fold: a table batch, its rows grouped by store
  FoldSegDev seg_dev;
  bool dedup;       // lcv_set_dedup: the chunks run the BLS half once per distinct item
  bool rlc;         // lcv_set_rlc: the batch-engine chunks pay one final exponentiation per group of items
};

// argument and state checks, the slot's work space, Params and the committee view
static int validate_prepare(lcv_ctx* ctx, lcv_dbatch* db, uint64_t current_slot, const uint8_t* gvr, const ValidateReq& q,
                            ValidateRun& v) {
  if (!ctx || !db || !gvr) return fail(ctx, LCV_EINVAL, "validate: null argument");
  const FoldReq* fold = q.fold;
  const FoldSegs* segs = fold ? fold->segs : nullptr;
  if (fold && !segs && db->B.store_index) return fail(ctx, LCV_EINVAL, "validate: no fold of a store-table batch");
  if (segs && !db->B.store_index) return fail(ctx, LCV_EINVAL, "validate: a segmented fold needs a store-table batch");
  if (fold && (db->n > LCV_FOLD_MAX_ROWS || db->n > ctx->chunk))
    return fail(ctx, LCV_EINVAL, "validate: a fold takes at most 65536 updates (one chunk) per call");
  // table: a batch that carries its store_index has every update validated against its own row of the store
  // table.  A resident batch outlives the table its indices were first checked against, so the largest index
  // (recorded with the column) is checked against the table of this call, on the host, before any launch
  const bool table = db->B.store_index != nullptr;
  if (table) {
    if (!ctx->table_set) return fail(ctx, LCV_ESTATE, "validate: lcv_set_store_table has not been called");
    if (db->max_store >= ctx->table_dev.nstore)
      return fail(ctx, LCV_EINVAL, "validate: the batch's largest store_index " + std::to_string(db->max_store) +
                                       " is not a store row of the current table (nstore " +
                                       std::to_string(ctx->table_dev.nstore) + ")");
  } else if (!ctx->store_set) {
    return fail(ctx, LCV_ESTATE, "validate: lcv_set_store has not been called");
  }
  v.ctx = ctx;
  v.db = db;
  v.q = q;
  v.async = q.slot >= 0;  // lcv_validate_resident_async: enqueue on the slot's streams, no wait
  v.slot = v.async ? q.slot : 0;
  v.n = db->n;
  if (v.async && v.n > ctx->chunk) return fail(ctx, LCV_EINVAL, "lcv_validate_resident_async: at most 65536 updates per call");
  v.cap = v.n < ctx->chunk ? v.n : ctx->chunk;
  be_set_slot(ctx, v.slot);
  int rc = ensure_work(ctx, v.cap, db->npool, v.slot);
  if (rc == LCV_OK && segs) rc = ensure_fold_seg(ctx, v.slot, segs->nseg);
  if (rc != LCV_OK) {
    be_set_slot(ctx, 0);
    return rc;
  }
  v.segs = segs;
  v.seg_dev = FoldSegDev{};
  if (segs) {
    v.seg_dev = fold->seg_dev;
    v.seg_dev.out = ctx->slot[v.slot].seg.p;
  }
  v.P.cfg = ctx->cfg;
  v.P.current_slot = current_slot;
  v.P.store_fin_slot = ctx->store_fin_slot;
  v.P.next_known = ctx->next_known;
  for (int k = 0; k < 8; ++k) v.P.gvr[k] = host_be32(gvr + 4 * k);
  // (the table path never reads the pool rows' store-equality flag: item_nsc_team gets a valid row to compare)
  v.C = table ? committee_view(ctx->table, ctx->table.raw.p) : committee_view(ctx->store, ctx->store.raw.p + K_SC);
  v.S = table ? &ctx->table_dev : nullptr;
  return LCV_OK;
}

// The rows and items of the batch, summed over its chunks for lcv_last_dedup (synchronous calls: slot 0), in
// one place.  bls_chunk: a chunk of a batch that has its grouping (staged) or its class column (resident) runs the
// BLS half once per distinct item under lcv_set_dedup; otherwise, and always with the mode off, once per row
static void count_items(ValidateRun& v, uint64_t rows, uint64_t items) {
  v.ctx->slot[v.slot].dd_rows += rows;
  v.ctx->slot[v.slot].dd_items += items;
}
// rlc_chunk: a chunk of `items` items on the batch engine under lcv_set_rlc gets the slot's scratch, the next batch
// counter and its groups counted for lcv_last_rlc (the batch's first chunk on a slot zeroes that slot's count of retried
// rows, every chunk the length of retry[]); else L stays null and the chunk runs as with the mode off
#if defined(LCV_CPU_FAST)
static bool rlc_on(const lcv_ctx*) { return false; }  // run_bls's direct branch runs every row: 0 groups
#else
static bool rlc_on(const lcv_ctx* ctx) { return ctx->rlc_group != 0; }
#endif
static int rlc_chunk(ValidateRun& v, int sl, uint32_t items, RlcRun& run, const RlcRun** L) {
  lcv_ctx* ctx = v.ctx;
  *L = nullptr;
  if (!v.rlc || items == 0 || fan_on(ctx, items)) return LCV_OK;
  LCV_TRY(ensure_rlc(ctx, sl));
  run.D = ctx->slot[sl].R;
  for (int k = 0; k < 8; ++k) run.key.seed[k] = ctx->rlc_seed[k];
  run.key.counter = ctx->rlc_counter++;
  run.shift = 0;
  while ((1u << run.shift) < ctx->rlc_group) ++run.shift;
  Slot& counted = ctx->slot[v.slot];
  const bool first = !(counted.rl_used & (1u << sl));
  LCV_TRY(be_memset(ctx, run.D.cnt, 0, first ? 2 * sizeof(uint32_t) : sizeof(uint32_t)));
  counted.rl_used |= 1u << sl;
  counted.rl_groups += (items + ctx->rlc_group - 1) / ctx->rlc_group;
  *L = &run;
  return LCV_OK;
}
static int bls_chunk(ValidateRun& v, int sl, const BatchDev& Bc, size_t base, uint32_t m, const BatchDev* nsc, bool rank) {
  RlcRun run;
  const RlcRun* L = nullptr;
  if (!v.dedup) {
    count_items(v, m, m);
    LCV_TRY(rlc_chunk(v, sl, m, run, &L));
    return run_bls(v.ctx, Bc, v.C, m, 0, &v.P, nsc, v.S, rank, nullptr, L);
  }
  DedupRun R;
  count_items(v, m, 0);  // (the rows count even where the grouping fails)
  LCV_TRY(dedup_chunk(v.ctx, v.db, sl, base, m, R));
  count_items(v, 0, R.m);
  LCV_TRY(rlc_chunk(v, sl, R.m, run, &L));
  return run_bls(v.ctx, Bc, v.C, m, 0, &v.P, nsc, v.S, rank, &R, L);
}

// what follows the verdicts of rows [base, base + m) in the active work space, on the main stream: the fold
// (after F_verdict in stream order on both engines, after every slice has joined under a pipeline; a segmented
// fold: one team per store present, each against its own row of the table), then the copies out
static int chunk_results(ValidateRun& v, size_t base, uint32_t m) {
  lcv_ctx* ctx = v.ctx;
  const ValidateReq& q = v.q;
  if (v.segs) LCV_TRY(fold_seg_stage(ctx, ctx->W, ctx->table_dev, v.seg_dev, v.segs->nseg));
  else if (q.fold) LCV_TRY(fold_stage(ctx, q.fold->in, v.P.store_fin_slot, v.P.next_known, m));
  if (!v.async && v.n <= v.cap && (q.verdict_host || q.reason_host || q.fold)) {
    // one chunk: both arrays (and a fold's result) into pinned memory without a wait each, handed out by
    // validate_finish after its sync
    HostSlot& h = ctx->hsync;
    const SlotResults r = {v.segs ? RES_FOLD_SEG : q.fold ? RES_FOLD : RES_VERDICTS, m, v.segs ? v.segs->nseg : 0u, 0};
    LCV_TRY(h.out.grow(ctx, results_offsets(r).total));
    LCV_TRY(results_enqueue(ctx, h.out.p, r, ctx->W, v.seg_dev.out, nullptr));
    h.res = r;
  } else {
    if (q.verdict_host) LCV_TRY(be_d2h(ctx, q.verdict_host + base, ctx->W.verdict, m));
    if (q.reason_host) LCV_TRY(be_d2h(ctx, q.reason_host + base, ctx->W.reason, m));
  }
  if (q.verdict_dev) LCV_TRY(be_d2d(ctx, q.verdict_dev + base, ctx->W.verdict, m));
  return LCV_OK;
}
// the end of a synchronous call: the wait, the results out of pinned memory, the stage timings
static int validate_finish(ValidateRun& v) {
  lcv_ctx* ctx = v.ctx;
  const ValidateReq& q = v.q;
  LCV_TRY(be_sync(ctx));
  const HostSlot& h = ctx->hsync;
  if (h.res.kind != RES_NONE)
    results_hand_out(h.out.p, h.res, v.segs ? v.segs->store.data() : nullptr, v.n, q.verdict_host, q.reason_host,
                     q.fold ? q.fold->out : nullptr, nullptr);
  be_collect_timings(ctx);
  return LCV_OK;
}

// Schedule 1, a synchronous batch of several chunks: the chunks rotate over the work-space slots, up to LCV_SLOTS
// in flight; a slot's results are copied out (waiting for it) before the slot takes its next chunk
static int validate_rotating(ValidateRun& v) {
  lcv_ctx* ctx = v.ctx;
  const ValidateReq& q = v.q;
  const size_t n = v.n, cap = v.cap, nchunks = (n + cap - 1) / cap;
  auto finish = [&](size_t c) -> int {
    const size_t base = c * cap;
    const uint32_t m = (uint32_t)((n - base) < cap ? (n - base) : cap);
    be_set_slot(ctx, (int)(c % LCV_SLOTS));
    const Work& Wc = ctx->slot[c % LCV_SLOTS].W;
    if (q.verdict_host) LCV_TRY(be_d2h(ctx, q.verdict_host + base, Wc.verdict, m));
    if (q.reason_host) LCV_TRY(be_d2h(ctx, q.reason_host + base, Wc.reason, m));
    if (q.verdict_dev) LCV_TRY(be_d2d(ctx, q.verdict_dev + base, Wc.verdict, m));
    return LCV_OK;
  };
  for (size_t c = 0; c < nchunks; ++c) {
    const int sl = (int)(c % LCV_SLOTS);
    if (c >= (size_t)LCV_SLOTS) LCV_TRY(finish(c - LCV_SLOTS));
    be_set_slot(ctx, sl);
    LCV_TRY(ensure_work(ctx, cap, v.db->npool, sl));
    const size_t base = c * cap;
    const uint32_t m = (uint32_t)((n - base) < cap ? (n - base) : cap);
    // every slot's first chunk also hashes the committee pool into that slot's work space
    LCV_TRY(bls_chunk(v, sl, chunk_view(v.db->B, base, m), base, m, c < (size_t)LCV_SLOTS ? &v.db->B : nullptr, false));
  }
  for (size_t c = nchunks > (size_t)LCV_SLOTS ? nchunks - LCV_SLOTS : 0; c < nchunks; ++c) LCV_TRY(finish(c));
  LCV_TRY(be_sync(ctx));
  be_collect_timings(ctx);
  return LCV_OK;
}

// Schedule 2, the sliced pipeline (lcv_set_pipeline, synchronous, never deduplicated): the committee roots come
// first; then each chunk is cut into pipe_chunks slices of a whole number of waves (64 items), whose chains
// (run_slice) are spread over `ns` streams.  A chunk too small to slice runs the two-stream schedule
static int validate_sliced(ValidateRun& v, int ns) {
  lcv_ctx* ctx = v.ctx;
  lcv_dbatch* db = v.db;
  const bool rank = v.q.fold != nullptr;
  LCV_TRY(stage(ctx, ST_NSC, [&] { return be_launch_team(ctx, F_nsc_team{db->B, v.C, ctx->W}, (uint32_t)db->npool); }));
  for (size_t base = 0; base < v.n; base += v.cap) {
    const uint32_t m = (uint32_t)((v.n - base) < v.cap ? (v.n - base) : v.cap);
    BatchDev B = chunk_view(db->B, base, m);
    if (m >= 128u * (uint32_t)ctx->pipe_chunks) {
      const uint32_t nc = (uint32_t)ctx->pipe_chunks;
      const uint32_t sl = ((m + nc - 1) / nc + 63u) & ~63u;
      count_items(v, m, m);
      for (int k = 1; k < ns; ++k) LCV_TRY(be_fork_to(ctx, k));
      uint32_t c = 0;
      for (uint32_t o = 0; o < m; o += sl, ++c) {
        const uint32_t len = (m - o) < sl ? (m - o) : sl;
        be_use_stream(ctx, (int)(c % (uint32_t)ns));
        const Work Wc = work_view(ctx->W, o);
        LCV_TRY(run_slice(ctx, chunk_view(B, o, len), v.C, v.P, v.S, Wc, len, rank));
      }
      // results leave from the main stream once every slice has joined: a copy to pageable host
      // memory on a slice's stream would block the host and serialise the slices
      be_use_stream(ctx, 0);
      for (int k = 1; k < ns; ++k) LCV_TRY(be_join_from(ctx, k));
    } else {
      LCV_TRY(bls_chunk(v, v.slot, B, base, m, nullptr, rank));
    }
    LCV_TRY(chunk_results(v, base, m));
  }
  return validate_finish(v);
}

// Schedule 3, one chunk on the two streams of its slot: synchronous on slot 0, or (async) enqueued on the caller's
// slot with no wait, the results left in the slot's work space
static int validate_single(ValidateRun& v) {
  const uint32_t m = (uint32_t)v.n;
  LCV_TRY(bls_chunk(v, v.slot, chunk_view(v.db->B, 0, m), 0, m, &v.db->B, v.q.fold != nullptr));
  LCV_TRY(chunk_results(v, 0, m));
  return v.async ? LCV_OK : validate_finish(v);
}

static int validate_impl(lcv_ctx* ctx, lcv_dbatch* db, uint64_t current_slot, const uint8_t* gvr, const ValidateReq& q) {
  ValidateRun v;
  LCV_TRY(validate_prepare(ctx, db, current_slot, gvr, q, v));
  if (!v.async) be_reset_timings(ctx);
  const int ns = ctx->pipe_streams < 4 ? ctx->pipe_streams : 4;  // lcv_set_pipeline: min(streams, 4)
  const bool piped = !v.async && ns > 1 && ctx->pipe_chunks > 1;
  v.dedup = dedup_on(ctx) && !piped && (db->plan_m > 0 || !db->cls.empty());
  Slot& s = ctx->slot[v.slot];
  s.dd_rows = s.dd_items = 0;
  v.rlc = rlc_on(ctx) && !piped;
  s.rl_groups = 0;
  s.rl_used = 0;
  const bool marks_were_off = ctx->marks_off;
  if (v.async) ctx->marks_off = true;  // nothing collects an asynchronous batch's stage marks
  // the pinned results of the slot's (synchronous: hsync's) last batch are no longer this batch's: the one-chunk
  // synchronous path and the enqueuing entries name the new ones once they are on their way
  (v.async ? s.host : ctx->hsync).res = SlotResults{};
  // (the boundary: a resident chunk's grouping under lcv_set_dedup allocates host memory, dedup_chunk)
  const int rc = guarded(ctx, "validate", [&] {
    return piped ? validate_sliced(v, ns) : (!v.async && v.n > v.cap) ? validate_rotating(v) : validate_single(v);
  });
  // whatever the schedule and its outcome: the caller's marks setting, slot 0 and its work space are the active ones again
  ctx->marks_off = marks_were_off;
  be_set_slot(ctx, 0);
  if (ctx->slot[0].work.p) ctx->W = ctx->slot[0].W;
  return rc;
}

int lcv_validate_resident(lcv_ctx* ctx, lcv_dbatch* db, uint64_t current_slot, const uint8_t* gvr, uint8_t* verdict_out,
                          uint8_t* reason_out) {
  ValidateReq q;
  q.verdict_host = verdict_out;
  q.reason_host = reason_out;
  return validate_impl(ctx, db, current_slot, gvr, q);
}

int lcv_validate_resident_dev(lcv_ctx* ctx, lcv_dbatch* db, uint64_t current_slot, const uint8_t* gvr,
                              uint8_t* verdict_dev) {
  ValidateReq q;
  q.verdict_dev = verdict_dev;
  return validate_impl(ctx, db, current_slot, gvr, q);
}

// Several batches in flight: the call enqueues the whole pipeline for `db` on the streams of work-space slot
// `slot` (0..7) and returns; lcv_slot_wait waits for that slot and copies its verdicts and reasons
// out.  A slot's next call starts on the device after its previous batch (stream order), so the
// caller alternates slots and waits for a slot before reusing it, as a double-buffered serving loop.
int lcv_validate_resident_async(lcv_ctx* ctx, lcv_dbatch* db, uint64_t current_slot, const uint8_t* gvr, int slot) {
  if (!ctx || slot < 0 || slot >= LCV_SLOTS) return fail(ctx, LCV_EINVAL, "lcv_validate_resident_async: slot must be 0..7");
  ValidateReq q;
  q.slot = slot;
  return validate_impl(ctx, db, current_slot, gvr, q);
}

// Host-input form of lcv_validate_resident_async (the serving path of SURVEY §8(d): host batch in, verdicts
// out).  The batch's columns are copied into the slot's pinned staging buffer (host threads), one DMA moves
// them to the slot's device copy on the slot's main stream — overlapping the kernels of the other slots'
// batches — then the whole pipeline is enqueued, and the verdicts and reasons are copied back into pinned
// host memory at the end of the slot's stream; lcv_slot_wait waits and hands them out.
// host copies of a staging step, on up to 4 host threads above 8 MB in all
struct CopyPiece { uint8_t* d; const uint8_t* s; size_t b; };
static void copy_pieces(const std::vector<CopyPiece>& pieces, size_t total) {
  const size_t nt = total >= ((size_t)8 << 20) ? 4 : 1;
  auto work = [&](size_t t) {
    for (size_t i = t; i < pieces.size(); i += nt) memcpy(pieces[i].d, pieces[i].s, pieces[i].b);
  };
  if (nt == 1) {
    work(0);
    return;
  }
  // an extern "C" entry point must not let an exception out: if a helper thread cannot be created, the
  // pieces it would have copied are copied here
  std::vector<std::thread> th;
  size_t started = 1;
  try {
    for (size_t t = 1; t < nt; ++t, ++started) th.emplace_back(work, t);
  } catch (...) {
  }
  work(0);
  for (size_t t = started; t < nt; ++t) work(t);
  for (auto& x : th) x.join();
}
// the columns of c into dst (laid out as c)
static void stage_columns(uint8_t* dst, const BatchCols& c) {
  std::vector<CopyPiece> pieces;
  const size_t kPiece = (size_t)1 << 20;
  for (int k = 0; k < BATCH_COLS; ++k)
    for (size_t o = 0; o < c.bytes[k]; o += kPiece)
      pieces.push_back({dst + c.off[k] + o, (const uint8_t*)c.src[k] + o, c.bytes[k] - o < kPiece ? c.bytes[k] - o : kPiece});
  copy_pieces(pieces, c.total);
}

// A one-chunk host batch into the HostSlot h (stage_transit): its columns, with a segmented fold's grouping `segs` and,
// under lcv_set_dedup, its grouping into BLS items, which both travel with the batch; h.db then names the device
// columns, and fold->seg_dev the grouping's.  `r`: what the batch's results will be (the enqueuing entries' h.out)
static int stage_host_batch(lcv_ctx* ctx, const char* who, const lcv_update_batch* hb, const uint32_t* store_index,
                            FoldReq* fold, int slot, HostSlot& h, SlotResults& r) {
  const FoldSegs* segs = fold ? fold->segs : nullptr;
  DedupCols dd;
  BatchCols c;
  LCV_TRY(dedup_stage(ctx, hb, store_index, dd));
  LCV_TRY(batch_cols(ctx, hb, c, who, store_index, segs, dd.m ? &dd : nullptr));
  r = {segs ? RES_FOLD_SEG : fold ? RES_FOLD : RES_VERDICTS, (size_t)c.n, segs ? segs->nseg : 0u, 0};
  LCV_TRY(stage_transit(ctx, slot, h, c.total, c.total, slot >= 0 ? results_offsets(r).total : 0,
                        [&](uint8_t* pin) { stage_columns(pin, c); }));
  bind_batch(&h.db, h.dev.p, c);
  if (segs) seg_bind(*fold, h.dev.p, c.off[COL_SEG_STORE], c.off[COL_SEG_OFF], c.off[COL_SEG_ROW], c.off[COL_SEG_IN]);
  return LCV_OK;
}

// The common tail of the enqueuing entries, the batch staged in ctx->slot[slot].host: the whole pipeline on the slot's
// streams (validate_impl), the results r on their way into the pinned region behind it, then the slot's record
static int slot_enqueue(lcv_ctx* ctx, int slot, uint64_t current_slot, const uint8_t* gvr, const FoldReq* fold,
                        const SlotResults& r, const uint8_t* rec) {
  Slot& s = ctx->slot[slot];
  HostSlot& h = s.host;
  ValidateReq q;
  q.slot = slot;
  q.fold = fold;
  LCV_TRY(validate_impl(ctx, &h.db, current_slot, gvr, q));
  be_set_slot(ctx, slot);
  const int rc = results_enqueue(ctx, h.out.p, r, s.W, s.seg.p, rec);
  be_set_slot(ctx, 0);
  if (rc != LCV_OK) return rc;
  if (r.by_store()) h.seg_store = fold->segs->store;  // (throws before the slot is marked: nothing a wait could scatter)
  h.res = r;
  return LCV_OK;
}

// every store_index of a host batch against the table that is set, naming the first offending row
static int store_index_check(lcv_ctx* ctx, const char* who, const uint32_t* store_index, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (store_index[i] >= ctx->table_dev.nstore)
      return fail(ctx, LCV_EINVAL, std::string(who) + ": store_index[" + std::to_string(i) + "] = " +
                                       std::to_string(store_index[i]) + " is not a store row (nstore " +
                                       std::to_string(ctx->table_dev.nstore) + ")");
  return LCV_OK;
}
// store_index null: against the context's store (lcv_validate_async); else row by row against the store table
// (lcv_validate_stores_async), the 14th column staged with the others
static int validate_async_host(lcv_ctx* ctx, const char* who, const lcv_update_batch* hb, const uint32_t* store_index,
                               uint64_t current_slot, const uint8_t* gvr, int slot, FoldReq* fold = nullptr) {
  return guarded(ctx, who, [&]() -> int {
    const FoldSegs* segs = fold ? fold->segs : nullptr;  // (a segmented fold's grouping has checked every index)
    if (store_index && !segs) LCV_TRY(store_index_check(ctx, who, store_index, hb->n));  // before the DMA
    SlotResults r;
    LCV_TRY(stage_host_batch(ctx, who, hb, store_index, fold, slot, ctx->slot[slot].host, r));
    return slot_enqueue(ctx, slot, current_slot, gvr, fold, r, nullptr);
  });
}

int lcv_validate_async(lcv_ctx* ctx, const lcv_update_batch* hb, uint64_t current_slot, const uint8_t* gvr, int slot) {
  if (!ctx || !hb || !gvr || slot < 0 || slot >= LCV_SLOTS)
    return fail(ctx, LCV_EINVAL, "lcv_validate_async: null argument or slot not in 0..7");
  if (!ctx->store_set) return fail(ctx, LCV_ESTATE, "lcv_validate_async: lcv_set_store has not been called");
  if (hb->n > ctx->chunk) return fail(ctx, LCV_EINVAL, "lcv_validate_async: at most 65536 updates per call");
  return validate_async_host(ctx, "lcv_validate_async", hb, nullptr, current_slot, gvr, slot);
}

int lcv_validate_stores_async(lcv_ctx* ctx, const lcv_update_batch* hb, const uint32_t* store_index,
                              uint64_t current_slot, const uint8_t* gvr, int slot) {
  if (!ctx || !hb || !store_index || !gvr || slot < 0 || slot >= LCV_SLOTS)
    return fail(ctx, LCV_EINVAL, "lcv_validate_stores_async: null argument or slot not in 0..7");
  if (!ctx->table_set) return fail(ctx, LCV_ESTATE, "lcv_validate_stores_async: lcv_set_store_table has not been called");
  if (hb->n > ctx->chunk) return fail(ctx, LCV_EINVAL, "lcv_validate_stores_async: at most 65536 updates per call");
  return validate_async_host(ctx, "lcv_validate_stores_async", hb, store_index, current_slot, gvr, slot);
}

// what every wait does behind its own argument and kind checks, for a slot whose results are on their way to pinned
// memory (h.res names them): the wait for the slot, then the hand-out of the first n rows and of what else is asked for
static int slot_collect(lcv_ctx* ctx, int slot, uint64_t n, uint8_t* verdict_out, uint8_t* reason_out,
                        lcv_fold_result* fold_out, uint8_t* status_out) {
  const HostSlot& h = ctx->slot[slot].host;
  if (n > h.res.n) return fail(ctx, LCV_EINVAL, "lcv_slot_wait: more rows than the slot's batch");
  be_set_slot(ctx, slot);
  const int rc = be_sync_slot(ctx);
  be_set_slot(ctx, 0);
  if (rc != LCV_OK) return rc;
  results_hand_out(h.out.p, h.res, h.seg_store.data(), (size_t)n, verdict_out, reason_out, fold_out, status_out);
  return LCV_OK;
}

int lcv_slot_wait(lcv_ctx* ctx, int slot, uint64_t n, uint8_t* verdict_out, uint8_t* reason_out) {
  if (!ctx || slot < 0 || slot >= LCV_SLOTS) return fail(ctx, LCV_EINVAL, "lcv_slot_wait: slot must be 0..7");
  Slot& s = ctx->slot[slot];
  // a host-input batch (lcv_validate_async) or a relay's: its results are already on their way to pinned memory
  if (s.host.res.kind != RES_NONE) return slot_collect(ctx, slot, n, verdict_out, reason_out, nullptr, nullptr);
  if (n > s.work.cap) return fail(ctx, LCV_EINVAL, "lcv_slot_wait: more rows than the slot holds");
  be_set_slot(ctx, slot);
  const Work& W = s.W;
  int rc = LCV_OK;
  if (n && verdict_out) rc = be_d2h(ctx, verdict_out, W.verdict, n);
  if (rc == LCV_OK && n && reason_out) rc = be_d2h(ctx, reason_out, W.reason, n);
  if (rc == LCV_OK) rc = be_sync_slot(ctx);
  be_set_slot(ctx, 0);
  return rc;
}

// host batch in, verdicts out, synchronous: against the context's store (store_index null) or, row by row,
// against the store table
static int validate_host(lcv_ctx* ctx, const lcv_update_batch* hb, const uint32_t* store_index, uint64_t current_slot,
                         const uint8_t* gvr, uint8_t* verdict_out, uint8_t* reason_out, FoldReq* fold = nullptr) {
  const bool table = store_index != nullptr;
  ValidateReq q;
  q.verdict_host = verdict_out;
  q.reason_host = reason_out;
  q.fold = fold;
  return guarded(ctx, "lcv_validate_updates", [&]() -> int {
    if (ctx && hb && gvr && (table ? ctx->table_set : ctx->store_set) && hb->n > 0 && hb->n <= ctx->chunk) {
      // one chunk (the reference's per-update call shape among them): staged like lcv_validate_async's, waited for here
      SlotResults r;  // (named again by chunk_results, with the batch on its way)
      LCV_TRY(stage_host_batch(ctx, "lcv_validate_updates", hb, store_index, fold, -1, ctx->hsync, r));
      return validate_impl(ctx, &ctx->hsync.db, current_slot, gvr, q);  // returns synced
    }
    if (fold) return fail(ctx, LCV_EINVAL, "lcv_validate_fold: null argument, no store set, or not 0 < n <= one chunk");
    // larger batches (and invalid arguments, reported by the upload): a device batch per call
    lcv_dbatch* db = nullptr;
    LCV_TRY(batch_upload(ctx, hb, store_index, &db));
    int rc = validate_impl(ctx, db, current_slot, gvr, q);
    lcv_batch_free(ctx, db);
    return rc;
  });
}

int lcv_validate_updates(lcv_ctx* ctx, const lcv_update_batch* hb, uint64_t current_slot, const uint8_t* gvr,
                         uint8_t* verdict_out, uint8_t* reason_out) {
  return validate_host(ctx, hb, nullptr, current_slot, gvr, verdict_out, reason_out);
}

// ---- the store fold (include/lcv.h; lcv_fold.hpp): lcv_validate_updates / lcv_validate_async with F_rank beside
// the pre-checks and F_fold behind the verdicts, the result travelling back with them
int lcv_validate_fold(lcv_ctx* ctx, const lcv_update_batch* hb, uint64_t current_slot, const uint8_t* gvr,
                      const lcv_fold_state* in, uint8_t* verdict_out, uint8_t* reason_out, lcv_fold_result* out) {
  if (!ctx || !hb || !gvr || !out) return fail(ctx, LCV_EINVAL, "lcv_validate_fold: null argument");
  if (!ctx->store_set) return fail(ctx, LCV_ESTATE, "lcv_validate_fold: lcv_set_store has not been called");
  if (hb->n == 0 || hb->n > LCV_FOLD_MAX_ROWS || hb->n > ctx->chunk)
    return fail(ctx, LCV_EINVAL, "lcv_validate_fold: need 0 < n <= 65536 (one chunk): cut larger batches and carry `next` forward");
  FoldReq req;
  LCV_TRY(fold_state_in(ctx, "lcv_validate_fold", in, req.in));
  req.out = out;
  return validate_host(ctx, hb, nullptr, current_slot, gvr, verdict_out, reason_out, &req);
}

int lcv_validate_async_fold(lcv_ctx* ctx, const lcv_update_batch* hb, uint64_t current_slot, const uint8_t* gvr,
                            const lcv_fold_state* in, int slot) {
  if (!ctx || !hb || !gvr || slot < 0 || slot >= LCV_SLOTS)
    return fail(ctx, LCV_EINVAL, "lcv_validate_async_fold: null argument or slot not in 0..7");
  if (!ctx->store_set) return fail(ctx, LCV_ESTATE, "lcv_validate_async_fold: lcv_set_store has not been called");
  if (hb->n == 0 || hb->n > LCV_FOLD_MAX_ROWS || hb->n > ctx->chunk)
    return fail(ctx, LCV_EINVAL, "lcv_validate_async_fold: need 0 < n <= 65536 (one chunk) per call");
  FoldReq req;
  LCV_TRY(fold_state_in(ctx, "lcv_validate_async_fold", in, req.in));
  req.out = nullptr;  // the result waits in the slot's pinned area for lcv_slot_wait_fold
  return validate_async_host(ctx, "lcv_validate_async_fold", hb, nullptr, current_slot, gvr, slot, &req);
}

int lcv_slot_wait_fold(lcv_ctx* ctx, int slot, uint64_t n, uint8_t* verdict_out, uint8_t* reason_out, lcv_fold_result* out) {
  if (!ctx || !out || slot < 0 || slot >= LCV_SLOTS) return fail(ctx, LCV_EINVAL, "lcv_slot_wait_fold: null argument or slot not in 0..7");
  if (ctx->slot[slot].host.res.kind != RES_FOLD)
    return fail(ctx, LCV_ESTATE, "lcv_slot_wait_fold: the slot's batch was not enqueued with a fold");
  return slot_collect(ctx, slot, n, verdict_out, reason_out, out, nullptr);
}

// test hook: F_fold alone on caller-supplied rank records and verdicts (no validation, no store)
int lcv_debug_fold(lcv_ctx* ctx, const uint8_t* rank, const uint8_t* verdict, uint64_t n, uint64_t store_finalized_slot,
                   int next_known, const lcv_fold_state* in, lcv_fold_result* out) {
  if (!ctx || !rank || !verdict || !out) return fail(ctx, LCV_EINVAL, "lcv_debug_fold: null argument");
  if (n == 0 || n > LCV_FOLD_MAX_ROWS) return fail(ctx, LCV_EINVAL, "lcv_debug_fold: need 0 < n <= 65536");
  FoldState s;
  LCV_TRY(fold_state_in(ctx, "lcv_debug_fold", in, s));
  // the three fields F_fold touches, in an allocation of their own (a whole work space of n rows is not needed)
  Layout l;
  const size_t o_rank = l.take(rank_index((size_t)n)), o_ver = l.take((size_t)n), o_out = l.total();
  Scratch mem(ctx);
  be_set_slot(ctx, 0);
  LCV_TRY(mem.alloc(o_out + FOLD_RESULT_BYTES));
  Work W = Work{};
  W.cap = (uint32_t)n;
  W.rank = mem.p + o_rank;
  W.verdict = mem.p + o_ver;
  W.fold_out = mem.p + o_out;
  be_reset_timings(ctx);
  FoldResult res;
  LCV_TRY(be_h2d(ctx, W.rank, rank, rank_index((size_t)n)));
  LCV_TRY(be_h2d(ctx, W.verdict, verdict, (size_t)n));
  LCV_TRY(stage(ctx, ST_FOLD, [&] {
    return be_launch_team(ctx, F_fold{W, s, store_finalized_slot, next_known ? 1u : 0u, (uint32_t)n}, 1);
  }));
  LCV_TRY(be_d2h(ctx, &res, W.fold_out, sizeof(res)));
  LCV_TRY(be_sync(ctx));
  mem.release();  // (waits for the streams)
  be_collect_timings(ctx);
  memcpy(out, &res, sizeof(res));
  return LCV_OK;
}

// the rank records of a host batch: only the six columns F_rank reads are looked at and uploaded (every other
// pointer of the batch may be null), in pieces of one chunk; no store, no work space
int lcv_rank_updates(lcv_ctx* ctx, const lcv_update_batch* hb, uint8_t* rank_out) {
  if (!ctx || !hb || !rank_out) return fail(ctx, LCV_EINVAL, "lcv_rank_updates: null argument");
  if (!hb->sync_bits || !hb->nsc_branch || !hb->finality_branch || !hb->attested.beacon || !hb->finalized.beacon ||
      !hb->signature_slot)
    return fail(ctx, LCV_EINVAL, "lcv_rank_updates: null column (sync_bits, nsc_branch, finality_branch, attested.beacon, "
                                 "finalized.beacon, signature_slot are read)");
  if (hb->n == 0 || hb->n > 0xffffffffull) return fail(ctx, LCV_EINVAL, "lcv_rank_updates: need 0 < n < 2^32");
  const size_t n = hb->n, piece = n < kChunk ? n : kChunk;
  const size_t width[6] = {K_BEACON, K_BEACON, K_NSC_BRANCH, K_FIN_BRANCH, 64, 8};
  const uint8_t* src[6] = {hb->attested.beacon, hb->finalized.beacon, hb->nsc_branch, hb->finality_branch, hb->sync_bits,
                           (const uint8_t*)hb->signature_slot};
  size_t off[7];
  Layout l;
  for (int k = 0; k < 7; ++k) off[k] = l.take((k < 6 ? width[k] : (size_t)RANK_BYTES) * piece);
  Scratch mem(ctx);
  be_set_slot(ctx, 0);
  LCV_TRY(mem.alloc(l.total()));
  uint8_t* m = mem.p;
  BatchDev B = {};
  B.att_beacon = m + off[0]; B.fin_beacon = m + off[1]; B.nsc_branch = m + off[2]; B.finality_branch = m + off[3];
  B.bits = m + off[4]; B.sig_slot = (const uint64_t*)(m + off[5]);
  Work W = Work{};
  W.rank = m + off[6];
  Params P = {};
  P.cfg = ctx->cfg;
  be_reset_timings(ctx);
  for (size_t base = 0; base < n; base += piece) {
    const size_t len = n - base < piece ? n - base : piece;
    for (int k = 0; k < 6; ++k) LCV_TRY(be_h2d(ctx, m + off[k], src[k] + width[k] * base, width[k] * len));
    B.n = (uint32_t)len;
    LCV_TRY(rank_stage(ctx, B, P, W, (uint32_t)len));
    LCV_TRY(be_d2h(ctx, rank_out + rank_index(base), W.rank, rank_index(len)));
    LCV_TRY(be_sync(ctx));  // the caller's pageable memory: each piece has left before the buffers are reused
  }
  be_collect_timings(ctx);
  return LCV_OK;  // (the scratch's free waits for the streams)
}

// ---- store table: a store snapshot per update (a catch-up over several sync-committee periods, whose updates
// each meet the store the previous ones left; or the updates of many light clients in one batch).  Every index
// a kernel follows is checked here, on the host, before anything is launched.
int lcv_set_store_table(lcv_ctx* ctx, const lcv_store_table* t, uint8_t* key_status_out) {
  if (!ctx || !t || !t->committees || !t->finalized_slot || !t->current || !t->next)
    return fail(ctx, LCV_EINVAL, "lcv_set_store_table: null argument");
  if (t->ncomm == 0 || t->ncomm > LCV_STORE_TABLE_MAX_COMMITTEES)
    return fail(ctx, LCV_EINVAL, "lcv_set_store_table: ncomm " + std::to_string(t->ncomm) + " is not in 1.." +
                                     std::to_string(LCV_STORE_TABLE_MAX_COMMITTEES));
  if (t->nstore == 0 || t->nstore > 0xffffffffull) return fail(ctx, LCV_EINVAL, "lcv_set_store_table: need 0 < nstore < 2^32");
  const size_t nc = t->ncomm, ns = t->nstore;
  for (size_t s = 0; s < ns; ++s) {
    if (t->current[s] >= nc)
      return fail(ctx, LCV_EINVAL, "lcv_set_store_table: current[" + std::to_string(s) + "] = " +
                                       std::to_string(t->current[s]) + " is not a committee row (ncomm " + std::to_string(nc) + ")");
    if (t->next[s] >= nc && t->next[s] != LCV_STORE_NEXT_UNKNOWN)
      return fail(ctx, LCV_EINVAL, "lcv_set_store_table: next[" + std::to_string(s) + "] = " + std::to_string(t->next[s]) +
                                       " is neither a committee row (ncomm " + std::to_string(nc) + ") nor LCV_STORE_NEXT_UNKNOWN");
  }
  return guarded(ctx, "lcv_set_store_table", [&]() -> int {
    // an all-zero committee as `next` means "not known" (is_next_sync_committee_known, sync-protocol.md:316-317):
    // decided once per committee row, here
    std::vector<uint8_t> zero_row(nc, 0);
    for (size_t c = 0; c < nc; ++c) {
      const uint8_t* row = t->committees + (size_t)K_SC * c;
      uint32_t any = 0;
      for (int k = 0; k < K_SC; ++k) any |= row[k];
      zero_row[c] = any ? 0 : 1;
    }
    Layout l;
    const size_t o_fin = l.take(8 * ns), o_cur = l.take(4 * ns), o_next = l.take(4 * ns);
    std::vector<uint32_t> next(ns);
    for (size_t s = 0; s < ns; ++s)
      next[s] = (t->next[s] == LCV_STORE_NEXT_UNKNOWN || zero_row[t->next[s]]) ? (uint32_t)STORE_NEXT_UNKNOWN : t->next[s];
    // the store columns also stay on the host, as the device gets them: lcv_set_dedup's grouping makes item_pre_table's
    // committee choice there (dedup_comm_rows)
    std::vector<uint64_t> host_fin(t->finalized_slot, t->finalized_slot + ns);
    std::vector<uint32_t> host_cur(t->current, t->current + ns);
    // drain: batches in flight on any work-space slot read the table's committees and store columns, so every
    // slot's streams are waited for before that memory is rewritten or freed.  A batch already enqueued thus
    // finishes under the table it was enqueued under; work enqueued after this call sees the new one
    be_set_slot(ctx, 0);
    LCV_TRY(be_sync(ctx));
    ctx->table_set = false;
    auto body = [&]() -> int {
      LCV_TRY(ensure_committees(ctx, ctx->table, nc, K_SC));
      LCV_TRY(ctx->table_mem.grow(ctx, ns, l.total()));
      uint8_t* m = ctx->table_mem.p;
      LCV_TRY(be_h2d(ctx, ctx->table.raw.p, t->committees, (size_t)K_SC * nc));
      LCV_TRY(be_h2d(ctx, m + o_fin, t->finalized_slot, 8 * ns));
      LCV_TRY(be_h2d(ctx, m + o_cur, t->current, 4 * ns));
      LCV_TRY(be_h2d(ctx, m + o_next, next.data(), 4 * ns));
      ctx->table_dev = StoreDev{(const uint64_t*)(m + o_fin), (const uint32_t*)(m + o_cur), (const uint32_t*)(m + o_next), (uint32_t)ns};
      be_reset_timings(ctx);
      LCV_TRY(build_committees(ctx, ctx->table));
      if (key_status_out) LCV_TRY(be_d2h(ctx, key_status_out, ctx->table.key_status.p, 512 * nc));
      return LCV_OK;
    };
    int rc = body();
    const int rs = be_sync(ctx);  // (also after a failure: `next` leaves scope with no copy pending)
    if (rc == LCV_OK) rc = rs;
    if (rc != LCV_OK) return rc;
    be_collect_timings(ctx);  // the table build's kernel time: lcv_last_timings' setup stage
    ctx->tab_fin.swap(host_fin);
    ctx->tab_cur.swap(host_cur);
    ctx->tab_next.swap(next);
    ctx->table_set = true;
    return LCV_OK;
  });
}

int lcv_validate_updates_stores(lcv_ctx* ctx, const lcv_update_batch* hb, const uint32_t* store_index,
                                uint64_t current_slot, const uint8_t* gvr, uint8_t* verdict_out, uint8_t* reason_out) {
  if (!ctx || !hb || !store_index || !gvr) return fail(ctx, LCV_EINVAL, "lcv_validate_updates_stores: null argument");
  if (!ctx->table_set) return fail(ctx, LCV_ESTATE, "lcv_validate_updates_stores: lcv_set_store_table has not been called");
  if (hb->n == 0 || hb->n > 0xffffffffull) return fail(ctx, LCV_EINVAL, "lcv_validate_updates_stores: need 0 < n < 2^32");
  LCV_TRY(store_index_check(ctx, "lcv_validate_updates_stores", store_index, hb->n));
  return validate_host(ctx, hb, store_index, current_slot, gvr, verdict_out, reason_out);
}

// ---- the fold of a store-table batch, store by store (include/lcv.h, "The segmented fold"; lcv_fold.hpp)
// store_index_check's pass, grouping as it goes: every index against nstore (naming the first offending row), and
// the rows keyed by (store, row).  Sorting the keys is the stable grouping — skipped when the rows already come
// store by store — so the cost is O(n log n) whatever the table's size, and nothing here is sized by nstore.
// Then the present stores' fold states are checked and gathered (in: indexed by store row).  Allocates host memory:
// within the boundary (guarded)
static int fold_segments(lcv_ctx* ctx, const char* who, const uint32_t* store_index, uint64_t n, uint64_t nstore,
                         const lcv_fold_state* in, FoldSegs& g) {
  g.key.resize(n);
  bool sorted = true;
  for (uint64_t i = 0; i < n; ++i) {
    if (store_index[i] >= nstore)
      return fail(ctx, LCV_EINVAL, std::string(who) + ": store_index[" + std::to_string(i) + "] = " +
                                       std::to_string(store_index[i]) + " is not a store row (nstore " +
                                       std::to_string(nstore) + ")");
    g.key[i] = ((uint64_t)store_index[i] << 32) | i;
    if (i && g.key[i] < g.key[i - 1]) sorted = false;
  }
  if (!sorted) std::sort(g.key.begin(), g.key.end());
  g.store.clear();
  g.off.clear();
  g.in.clear();
  g.row.resize(n);
  for (uint64_t j = 0; j < n; ++j) {
    const uint32_t s = (uint32_t)(g.key[j] >> 32);
    if (j == 0 || s != g.store.back()) {
      g.store.push_back(s);
      g.off.push_back((uint32_t)j);
    }
    g.row[j] = (uint32_t)g.key[j];
  }
  g.off.push_back((uint32_t)n);
  g.nseg = (uint32_t)g.store.size();
  g.in.resize(g.nseg);
  for (uint32_t k = 0; k < g.nseg; ++k)
    LCV_TRY(fold_state_in(ctx, (std::string(who) + ": in[" + std::to_string(g.store[k]) + "]").c_str(), &in[g.store[k]], g.in[k]));
  return LCV_OK;
}

int lcv_validate_stores_fold(lcv_ctx* ctx, const lcv_update_batch* hb, const uint32_t* store_index, uint64_t current_slot,
                             const uint8_t* gvr, const lcv_fold_state* in, uint8_t* verdict_out, uint8_t* reason_out,
                             lcv_fold_result* out) {
  if (!ctx || !hb || !store_index || !gvr || !in || !out) return fail(ctx, LCV_EINVAL, "lcv_validate_stores_fold: null argument");
  if (hb->n == 0 || hb->n > LCV_FOLD_MAX_ROWS || hb->n > ctx->chunk)
    return fail(ctx, LCV_EINVAL, "lcv_validate_stores_fold: need 0 < n <= 65536 (one chunk): cut larger batches and carry each store's `next` forward");
  if (!ctx->table_set) return fail(ctx, LCV_ESTATE, "lcv_validate_stores_fold: lcv_set_store_table has not been called");
  return guarded(ctx, "lcv_validate_stores_fold", [&]() -> int {
    LCV_TRY(fold_segments(ctx, "lcv_validate_stores_fold", store_index, hb->n, ctx->table_dev.nstore, in, ctx->segs));
    FoldReq req;
    req.in = FoldState{};
    req.out = out;
    req.segs = &ctx->segs;
    return validate_host(ctx, hb, store_index, current_slot, gvr, verdict_out, reason_out, &req);
  });
}

int lcv_validate_stores_async_fold(lcv_ctx* ctx, const lcv_update_batch* hb, const uint32_t* store_index,
                                   uint64_t current_slot, const uint8_t* gvr, const lcv_fold_state* in, int slot) {
  if (!ctx || !hb || !store_index || !gvr || !in || slot < 0 || slot >= LCV_SLOTS)
    return fail(ctx, LCV_EINVAL, "lcv_validate_stores_async_fold: null argument or slot not in 0..7");
  if (hb->n == 0 || hb->n > LCV_FOLD_MAX_ROWS || hb->n > ctx->chunk)
    return fail(ctx, LCV_EINVAL, "lcv_validate_stores_async_fold: need 0 < n <= 65536 (one chunk) per call");
  if (!ctx->table_set) return fail(ctx, LCV_ESTATE, "lcv_validate_stores_async_fold: lcv_set_store_table has not been called");
  return guarded(ctx, "lcv_validate_stores_async_fold", [&]() -> int {
    LCV_TRY(fold_segments(ctx, "lcv_validate_stores_async_fold", store_index, hb->n, ctx->table_dev.nstore, in, ctx->segs));
    FoldReq req;
    req.in = FoldState{};
    req.out = nullptr;  // the results wait in the slot's pinned area for lcv_slot_wait_stores_fold
    req.segs = &ctx->segs;
    return validate_async_host(ctx, "lcv_validate_stores_async_fold", hb, store_index, current_slot, gvr, slot, &req);
  });
}

int lcv_slot_wait_stores_fold(lcv_ctx* ctx, int slot, uint64_t n, uint8_t* verdict_out, uint8_t* reason_out,
                              lcv_fold_result* out) {
  if (!ctx || !out || slot < 0 || slot >= LCV_SLOTS)
    return fail(ctx, LCV_EINVAL, "lcv_slot_wait_stores_fold: null argument or slot not in 0..7");
  if (ctx->slot[slot].host.res.kind != RES_FOLD_SEG)
    return fail(ctx, LCV_ESTATE, "lcv_slot_wait_stores_fold: the slot's batch was not enqueued by lcv_validate_stores_async_fold");
  return slot_collect(ctx, slot, n, verdict_out, reason_out, out, nullptr);
}

// test hook: F_fold_seg alone on caller-supplied rank records, verdicts, store rows and per-store values (no
// validation, no table: the two store columns the kernel reads are built here, next_known[s] != 0 as a known row)
int lcv_debug_fold_stores(lcv_ctx* ctx, const uint8_t* rank, const uint8_t* verdict, const uint32_t* store_index, uint64_t n,
                          const uint64_t* store_finalized_slot, const uint8_t* next_known, uint64_t nstore,
                          const lcv_fold_state* in, lcv_fold_result* out) {
  if (!ctx || !rank || !verdict || !store_index || !store_finalized_slot || !next_known || !in || !out)
    return fail(ctx, LCV_EINVAL, "lcv_debug_fold_stores: null argument");
  if (n == 0 || n > LCV_FOLD_MAX_ROWS) return fail(ctx, LCV_EINVAL, "lcv_debug_fold_stores: need 0 < n <= 65536");
  if (nstore == 0 || nstore > 0xffffffffull) return fail(ctx, LCV_EINVAL, "lcv_debug_fold_stores: need 0 < nstore < 2^32");
  return guarded(ctx, "lcv_debug_fold_stores", [&]() -> int {
    FoldSegs& g = ctx->segs;
    LCV_TRY(fold_segments(ctx, "lcv_debug_fold_stores", store_index, n, nstore, in, g));
    std::vector<uint32_t> next(nstore);
    std::vector<uint8_t> res((size_t)FOLD_RESULT_BYTES * g.nseg);
    for (uint64_t s = 0; s < nstore; ++s) next[s] = next_known[s] ? 0u : (uint32_t)STORE_NEXT_UNKNOWN;
    const size_t ng = g.nseg;
    const void* src[8] = {rank, verdict, store_finalized_slot, next.data(), g.store.data(), g.off.data(), g.row.data(), g.in.data()};
    const size_t bytes[8] = {rank_index((size_t)n), (size_t)n, 8 * (size_t)nstore, 4 * (size_t)nstore, 4 * ng, 4 * (ng + 1),
                             4 * (size_t)n, sizeof(FoldState) * ng};
    size_t off[9];
    Layout l;
    for (int k = 0; k < 9; ++k) off[k] = l.take(k < 8 ? bytes[k] : (size_t)FOLD_RESULT_BYTES * ng);
    Scratch mem(ctx);
    be_set_slot(ctx, 0);
    LCV_TRY(mem.alloc(l.total()));
    uint8_t* m = mem.p;
    Work W = Work{};
    W.cap = (uint32_t)n;
    W.rank = m + off[0];
    W.verdict = m + off[1];
    const StoreDev S = {(const uint64_t*)(m + off[2]), nullptr, (const uint32_t*)(m + off[3]), (uint32_t)nstore};
    const FoldSegDev G = {(const uint32_t*)(m + off[4]), (const uint32_t*)(m + off[5]), (const uint32_t*)(m + off[6]),
                          m + off[7], m + off[8]};
    be_reset_timings(ctx);
    for (int k = 0; k < 8; ++k) LCV_TRY(be_h2d(ctx, m + off[k], src[k], bytes[k]));
    LCV_TRY(fold_seg_stage(ctx, W, S, G, g.nseg));
    LCV_TRY(be_d2h(ctx, res.data(), G.out, res.size()));
    LCV_TRY(be_sync(ctx));
    mem.release();  // (waits for the streams)
    be_collect_timings(ctx);
    fold_seg_scatter(out, res.data(), g.store.data(), g.nseg);
    return LCV_OK;
  });
}

// The communication buffer never blocks a collective call: lcv_comm_init sizes it for every slot's largest
// all-gather (a 64k-row chunk per rank, comm_buf_bytes_for), and a call that needs more (a sharded batch of
// several chunks per rank, or one re-sharded over fewer survivors) grows it WITHOUT freeing the old buffer —
// be_free synchronises every stream with no bound, and behind a collective on a dead peer that is forever
// (the bounded be_comm_wait comes later).  Outgrown buffers are retired and freed by lcv_destroy; growth is
// geometric, so a context retires O(log n) of them.
static size_t comm_buf_bytes_for(size_t nranks) { return kChunk * (nranks + 1) * LCV_SLOTS; }
static int ensure_comm_buf(lcv_ctx* ctx, const char* who, size_t bytes) {
  if (ctx->comm_buf.p && bytes <= ctx->comm_buf.cap) return LCV_OK;
  bytes = std::max(bytes, 2 * ctx->comm_buf.cap);  // doubles
  return guarded(ctx, who, [&]() -> int {
    ctx->comm_retired.reserve(ctx->comm_retired.size() + 1);  // (may throw: ahead of the allocation)
    DevBuf fresh;
    LCV_TRY(fresh.grow(ctx, bytes));
    if (ctx->comm_buf.p) ctx->comm_retired.push_back(ctx->comm_buf);  // retired, not freed
    ctx->comm_buf = fresh;
    return LCV_OK;
  });
}

// ---- multi-GPU: updates are sharded by contiguous index range, one process (and context) per GPU; the
// only collective is the all-gather of the per-update verdict bytes (SURVEY.md §8(e)).
int lcv_comm_unique_id(uint8_t* id128) {
  if (!id128) return LCV_EINVAL;
  return be_comm_unique_id(id128);
}

int lcv_comm_init(lcv_ctx* ctx, int nranks, int rank, const uint8_t* id128) {
  if (!ctx || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, LCV_EINVAL, "lcv_comm_init: bad arguments");
  if (ctx->comm_ready) return fail(ctx, LCV_ESTATE, "lcv_comm_init: communicator already initialised");
  LCV_TRY(be_comm_init(ctx, nranks, rank, id128));
  // every per-slot all-gather of up to a chunk per rank fits from the start (ensure_comm_buf)
  LCV_TRY(ensure_comm_buf(ctx, "lcv_comm_init", comm_buf_bytes_for((size_t)nranks)));
  ctx->comm_ready = true;
  ctx->comm_nranks = nranks;
  ctx->comm_rank = rank;
  return LCV_OK;
}

// the collectives' completion bound (lcv_comm_set_timeout) and the recovery entries: a failed
// communicator is shrunk to the surviving ranks (every survivor passes the same exclude list) or aborted
static int comm_usable(lcv_ctx* ctx, const char* what) {
  if (!ctx->comm_ready) return fail(ctx, LCV_ESTATE, std::string(what) + ": lcv_comm_init has not been called");
  if (ctx->comm_failed)
    return fail(ctx, LCV_ESTATE, std::string(what) + ": the communicator failed; lcv_comm_shrink or lcv_comm_abort first");
  return LCV_OK;
}

int lcv_comm_set_timeout(lcv_ctx* ctx, double seconds) {
  if (!ctx || !(seconds > 0.0)) return fail(ctx, LCV_EINVAL, "lcv_comm_set_timeout: seconds > 0");
  ctx->comm_timeout_s = seconds;
  return LCV_OK;
}

int lcv_comm_shrink(lcv_ctx* ctx, const int* exclude, int nexclude, int* new_rank, int* new_nranks) {
  if (!ctx || (nexclude && !exclude) || nexclude < 0 || !new_rank || !new_nranks)
    return fail(ctx, LCV_EINVAL, "lcv_comm_shrink: bad arguments");
  if (!ctx->comm_ready) return fail(ctx, LCV_ESTATE, "lcv_comm_shrink: lcv_comm_init has not been called");
  for (int i = 0; i < nexclude; ++i) {
    if (exclude[i] < 0 || exclude[i] >= ctx->comm_nranks || exclude[i] == ctx->comm_rank)
      return fail(ctx, LCV_EINVAL, "lcv_comm_shrink: an excluded rank is out of range or this rank");
    for (int j = 0; j < i; ++j)
      if (exclude[j] == exclude[i]) return fail(ctx, LCV_EINVAL, "lcv_comm_shrink: an excluded rank listed twice");
  }
  int rank = 0, n = 0;
  const int rc = be_comm_shrink(ctx, exclude, nexclude, &rank, &n);
  if (rc != LCV_OK) {
    be_comm_abort(ctx);
    ctx->comm_ready = false;
    ctx->comm_failed = false;
    return rc;
  }
  ctx->comm_rank = rank;
  ctx->comm_nranks = n;
  ctx->comm_failed = false;
  *new_rank = rank;
  *new_nranks = n;
  return LCV_OK;
}

int lcv_comm_abort(lcv_ctx* ctx) {
  if (!ctx) return LCV_EINVAL;
  if (ctx->comm_ready) be_comm_abort(ctx);
  ctx->comm_ready = false;
  ctx->comm_failed = false;
  return LCV_OK;
}

int lcv_comm_count(lcv_ctx* ctx, int* nranks_out) {
  if (!ctx || !nranks_out) return fail(ctx, LCV_EINVAL, "lcv_comm_count: null argument");
  if (!ctx->comm_ready) return fail(ctx, LCV_ESTATE, "lcv_comm_count: lcv_comm_init has not been called");
  return be_comm_count(ctx, nranks_out);
}

int lcv_comm_destroy(lcv_ctx* ctx) {
  if (!ctx) return LCV_EINVAL;
  if (ctx->comm_ready) {
    if (ctx->comm_failed) be_comm_abort(ctx);  // a failed communicator may never complete a destroy
    else be_comm_destroy(ctx);
  }
  ctx->comm_ready = false;
  ctx->comm_failed = false;
  return LCV_OK;
}

// This rank validates its resident shard (n <= per_rank rows) into a device slice of per_rank bytes
// (zero padded), then every rank's slice is all-gathered (RCCL, device to device) and the
// nranks * per_rank verdict bytes come back to the host: one sharded validate step.
// the all-gather of the verdicts of slot `slot`'s batch (lcv_validate_resident_async): after that batch on
// its main stream, into a per-slot region of the communication buffer; waits and copies to the host
int lcv_slot_allgather(lcv_ctx* ctx, int slot, uint64_t n, uint64_t per_rank, uint8_t* verdict_all_out) {
  if (!ctx || !verdict_all_out || slot < 0 || slot >= LCV_SLOTS) return fail(ctx, LCV_EINVAL, "lcv_slot_allgather: bad arguments");
  LCV_TRY(comm_usable(ctx, "lcv_slot_allgather"));
  if (n > per_rank || n > ctx->slot[slot].work.cap)
    return fail(ctx, LCV_EINVAL, "lcv_slot_allgather: n larger than per_rank or than the slot's batch");
  const size_t R = (size_t)ctx->comm_nranks, region = per_rank * (R + 1);
  LCV_TRY(ensure_comm_buf(ctx, "lcv_slot_allgather", region * LCV_SLOTS));
  uint8_t* send = ctx->comm_buf.p + region * (size_t)slot;
  uint8_t* recv = send + per_rank;
  ctx->slot[slot].host.res = SlotResults{};  // this slot's results leave through the all-gather
  be_set_slot(ctx, slot);
  int rc = be_memset(ctx, send, 0, per_rank);
  if (rc == LCV_OK && n) rc = be_d2d(ctx, send, ctx->slot[slot].W.verdict, n);
  if (rc == LCV_OK) rc = be_comm_allgather(ctx, send, recv, per_rank);
  // bounded: a dead peer fails the call instead of hanging it.  The wait comes BEFORE the copy into the
  // caller's (pageable) memory: such a copy blocks the host until the stream reaches it, i.e. forever
  // behind a collective that cannot complete
  if (rc == LCV_OK) rc = be_comm_wait(ctx);
  if (rc == LCV_OK) rc = be_d2h(ctx, verdict_all_out, recv, per_rank * R);
  if (rc == LCV_OK) rc = be_sync_slot(ctx);
  be_set_slot(ctx, 0);
  return rc;
}

int lcv_validate_sharded(lcv_ctx* ctx, lcv_dbatch* db, uint64_t current_slot, const uint8_t* gvr, uint64_t per_rank,
                         uint8_t* verdict_all_out) {
  if (!ctx || !db || !gvr || !verdict_all_out) return fail(ctx, LCV_EINVAL, "lcv_validate_sharded: null argument");
  LCV_TRY(comm_usable(ctx, "lcv_validate_sharded"));
  if (db->n > per_rank) return fail(ctx, LCV_EINVAL, "lcv_validate_sharded: shard larger than per_rank");
  const size_t R = (size_t)ctx->comm_nranks;
  LCV_TRY(ensure_comm_buf(ctx, "lcv_validate_sharded", per_rank * (R + 1)));
  uint8_t* send = ctx->comm_buf.p;
  uint8_t* recv = send + per_rank;
  // only the padding tail is zeroed: the verdicts [0, n) are written by the chunks' own slot streams
  // (validate_rotating), which nothing orders after a memset on this stream
  LCV_TRY(be_memset(ctx, send + db->n, 0, per_rank - db->n));
  ValidateReq q;
  q.verdict_dev = send;
  LCV_TRY(validate_impl(ctx, db, current_slot, gvr, q));
  LCV_TRY(be_comm_allgather(ctx, send, recv, per_rank));
  LCV_TRY(be_comm_wait(ctx));  // bounded, and before the copy into pageable caller memory (lcv_slot_allgather)
  LCV_TRY(be_d2h(ctx, verdict_all_out, recv, per_rank * R));
  return be_sync(ctx);
}

// max over ranks of one double per rank (in place); also a barrier of the communicator
int lcv_comm_allreduce_max(lcv_ctx* ctx, double* inout) {
  if (!ctx || !inout) return fail(ctx, LCV_EINVAL, "lcv_comm_allreduce_max: null argument");
  LCV_TRY(comm_usable(ctx, "lcv_comm_allreduce_max"));
  return be_comm_allreduce_max(ctx, inout);
}

// test hook: the size of the context's HIP event pool (asynchronous calls must not grow it)
int lcv_debug_event_pool(lcv_ctx* ctx, uint64_t* events_out) {
  if (!ctx || !events_out) return LCV_EINVAL;
  *events_out = (uint64_t)be_event_pool_size(ctx);
  return LCV_OK;
}

// test hook: validate cuts batches into chunks of `rows` (default 65536), so the chunk rotation over the work-space
// slots runs at host-simulation sizes.  Any size works: every chunk starts at item 0 of its slot's work space (the
// sliced pipeline rounds its slices to whole waves itself); sizes that are no multiple of a group give the batch
// verification's groups (lcv_set_rlc) a short tail in every chunk
int lcv_debug_set_chunk(lcv_ctx* ctx, uint64_t rows) {
  if (!ctx || rows < 1 || rows > 65536) return fail(ctx, LCV_EINVAL, "lcv_debug_set_chunk: 1 <= rows <= 65536");
  ctx->chunk = (size_t)rows;
  return LCV_OK;
}

// ---- work-space layout check (test entry; host arithmetic only, nothing is read or written on the device), over
// kWorkFields and kDedupFields: element r of item i of a field at base + field_index(i, r), the kernels' own functions.
// (1) work_view is derived from the same rows and functions, so what this proves is that every kind's index function
// is additive in the item — index(b + j, r) - index(j, r) depends on neither j nor r — the precondition of slicing by
// advancing a pointer.  It does not cross-check two hand-written lists, and it cannot see a field given the wrong
// kind in the table: the slices then overwrite each other's items on the device, where they run side by side (the
// sliced cases of tests/stage_mark_cases.py), but not on the host simulation, which runs them one after another.
// (2) proves the allocation: no two arrays of any slots overlap
static const uint8_t* field_addr(const void* obj, const Field& f, size_t cap, size_t pool_cap, size_t i, size_t r) {
  return slot_get(obj, f.slot) + f.esize * field_index(f, cap, pool_cap, i, r);
}

static int work_check(lcv_ctx* ctx, uint64_t cap, uint64_t slice, int nslots);
extern "C" int lcv_debug_work_check(lcv_ctx* ctx, uint64_t cap, uint64_t slice, int nslots) {
  if (!ctx || cap == 0 || slice == 0 || nslots < 1 || nslots > LCV_SLOTS)
    return fail(ctx, LCV_EINVAL, "lcv_debug_work_check: cap, slice > 0, 1 <= nslots <= 8");
  return guarded(ctx, "lcv_debug_work_check", [&] { return work_check(ctx, cap, slice, nslots); });
}
static int work_check(lcv_ctx* ctx, uint64_t cap, uint64_t slice, int nslots) {
  for (int s = 0; s < nslots; ++s) {
    LCV_TRY(ensure_work(ctx, cap, 5, s));  // a committee pool of 5
    LCV_TRY(ensure_dedup(ctx, cap, s));    // and the slot's deduplication scratch (lcv_set_dedup), checked in (2)
    LCV_TRY(ensure_rlc(ctx, s));           // and its batch-verification scratch (lcv_set_rlc), likewise
  }
  ctx->W = ctx->slot[0].W;
  // (1) slices: item j of work_view(W, b) is item b + j of W, element for element, in every per-item field
  for (int s = 0; s < nslots; ++s) {
    const Work& W = ctx->slot[s].W;
    const size_t C = W.cap, Pc = W.pool_cap;
    for (size_t b = 0; b < C; b += slice) {
      const Work V = work_view(W, b);
      const size_t len = C - b < slice ? C - b : slice;
      for (const Field& f : kWorkFields)
        if (field_per_item(f))
          for (size_t j = 0; j < len; ++j)
            for (size_t r = 0; r < f.rows; ++r)
              if (field_addr(&V, f, C, Pc, j, r) != field_addr(&W, f, C, Pc, b + j, r))
                return fail(ctx, LCV_EINVAL, std::string("lcv_debug_work_check: slot ") + std::to_string(s) + " field " +
                                                 f.name + ": item " + std::to_string(j) + " of the slice at " +
                                                 std::to_string(b) + " is not item " + std::to_string(b + j));
    }
  }
  // (2) every field of every slot: its byte range [first element, last element] is disjoint from every
  // other field's (of this slot and of the other slots), and every item's elements lie in it (the
  // committee-pool fields over their pool_cap items)
  struct Range { const uint8_t *lo, *hi; int slot; std::string name; };
  std::vector<Range> rg;
  auto ranges = [&](int s, const void* obj, const Field& f, const char* prefix, size_t C, size_t Pc) {
    const uint8_t* lo = field_addr(obj, f, C, Pc, 0, 0);
    const uint8_t* hi = lo;
    for (size_t i = 0; i < field_items(f, C, Pc); ++i)
      for (size_t r = 0; r < f.rows; ++r) {
        const uint8_t* a = field_addr(obj, f, C, Pc, i, r);
        if (a < lo) lo = a;
        if (a + f.esize > hi) hi = a + f.esize;
      }
    rg.push_back({lo, hi, s, std::string(prefix) + f.name});
  };
  for (int s = 0; s < nslots; ++s) {
    const Work& W = ctx->slot[s].W;
    for (const Field& f : kWorkFields) ranges(s, &W, f, "", W.cap, W.pool_cap);
    for (const Field& f : kDedupFields) ranges(s, &ctx->slot[s].D, f, "dedup_", W.cap, 0);
    for (const Field& f : kRlcFields) ranges(s, &ctx->slot[s].R, f, "rlc_", W.cap, 0);
  }
  for (size_t a = 0; a < rg.size(); ++a)
    for (size_t b = a + 1; b < rg.size(); ++b)
      if (rg[a].lo < rg[b].hi && rg[b].lo < rg[a].hi)
        return fail(ctx, LCV_EINVAL, std::string("lcv_debug_work_check: slot ") + std::to_string(rg[a].slot) + " " +
                                         rg[a].name + " overlaps slot " + std::to_string(rg[b].slot) + " " + rg[b].name);
  return LCV_OK;
}

int lcv_build_id(char* out, uint64_t cap) {
  const size_t n = strlen(LCV_BUILD_ID) + 1;
  if (!out || cap < n) return LCV_EINVAL;
  memcpy(out, LCV_BUILD_ID, n);
  return LCV_OK;
}

int lcv_set_latency_mode(lcv_ctx* ctx, uint64_t max_rows) {
  if (!ctx || max_rows > 65536) return fail(ctx, LCV_EINVAL, "lcv_set_latency_mode: max_rows <= 65536");
  ctx->fan_max = max_rows;
  return LCV_OK;
}

int lcv_debug_engine_log(lcv_ctx* ctx, uint64_t* out8, int reset) {
  if (!ctx || !out8) return LCV_EINVAL;
  for (int k = 0; k < 4; ++k) out8[k] = ctx->eng_count[k];
  for (int k = 0; k < 4; ++k) out8[4 + k] = ctx->eng_items[k];
  if (reset) {
    for (int k = 0; k < 4; ++k) ctx->eng_count[k] = 0;
    for (int k = 0; k < 4; ++k) ctx->eng_items[k] = 0;
  }
  return LCV_OK;
}

int lcv_set_pipeline(lcv_ctx* ctx, int streams, int chunks) {
  if (!ctx || streams < 1 || chunks < 1 || chunks > 4096) return fail(ctx, LCV_EINVAL, "lcv_set_pipeline: streams >= 1, 1 <= chunks <= 4096");
  if (streams > 1 && ctx->dedup)
    return fail(ctx, LCV_EINVAL, "lcv_set_pipeline: no multi-stream pipeline while lcv_set_dedup is on (sliced chains would need a grouping per slice)");
  if (streams > 1 && ctx->rlc_group)
    return fail(ctx, LCV_EINVAL, "lcv_set_pipeline: no multi-stream pipeline while lcv_set_rlc is on (the sliced chains run every row)");
  ctx->pipe_streams = streams < 4 ? streams : 4;
  ctx->pipe_chunks = chunks;
  return LCV_OK;
}

// ---- randomised batch verification (include/lcv.h "Batch verification")
int lcv_set_rlc(lcv_ctx* ctx, uint32_t group, const uint8_t* seed32) {
  if (!ctx) return LCV_EINVAL;
  if (group == 0) {
    ctx->rlc_group = 0;
    return LCV_OK;
  }
  if (group < 2 || group > 64 || (group & (group - 1)))
    return fail(ctx, LCV_EINVAL, "lcv_set_rlc: group must be 0 (off), 2, 4, 8, 16, 32 or 64");
  uint32_t any = 0;
  for (int k = 0; seed32 && k < 32; ++k) any |= seed32[k];
  if (!any) return fail(ctx, LCV_EINVAL, "lcv_set_rlc: the seed must be 32 bytes that are not all zero");
  if (ctx->pipe_streams > 1)
    return fail(ctx, LCV_EINVAL, "lcv_set_rlc: not with a multi-stream pipeline (lcv_set_pipeline streams > 1): the sliced chains run every row");
  for (int k = 0; k < 8; ++k) ctx->rlc_seed[k] = host_be32(seed32 + 4 * k);
  ctx->rlc_seeded = true;
  ctx->rlc_group = group;
  return LCV_OK;
}

// the retried rows are counted on the device, in the scratch of every slot the batch's chunks ran on: one small
// blocking read each, here and not on the asynchronous path
int lcv_last_rlc(lcv_ctx* ctx, int slot, uint64_t* groups, uint64_t* retried_rows) {
  if (!ctx || slot < 0 || slot >= LCV_SLOTS) return fail(ctx, LCV_EINVAL, "lcv_last_rlc: slot must be 0..7");
  if (groups) *groups = ctx->slot[slot].rl_groups;
  if (!retried_rows) return LCV_OK;
  uint64_t total = 0;
  int rc = LCV_OK;
  for (int s = 0; s < LCV_SLOTS && rc == LCV_OK; ++s) {
    if (!(ctx->slot[slot].rl_used & (1u << s)) || !ctx->slot[s].rlc.p) continue;
    uint32_t c = 0;
    be_set_slot(ctx, s);
    rc = be_d2h(ctx, &c, ctx->slot[s].R.cnt + 1, sizeof(c));
    if (rc == LCV_OK) rc = be_sync_slot(ctx);
    total += c;
  }
  be_set_slot(ctx, 0);
  *retried_rows = total;
  return rc;
}

// ---- deduplicated BLS half (include/lcv.h "Deduplicated signatures")
int lcv_set_dedup(lcv_ctx* ctx, int on) {
  if (!ctx) return LCV_EINVAL;
  if (on && ctx->pipe_streams > 1)
    return fail(ctx, LCV_EINVAL, "lcv_set_dedup: not with a multi-stream pipeline (lcv_set_pipeline streams > 1): sliced chains would need a grouping per slice");
  ctx->dedup = on != 0;
  return LCV_OK;
}

int lcv_last_dedup(lcv_ctx* ctx, int slot, uint64_t* rows, uint64_t* items) {
  if (!ctx || slot < 0 || slot >= LCV_SLOTS) return fail(ctx, LCV_EINVAL, "lcv_last_dedup: slot must be 0..7");
  if (rows) *rows = ctx->slot[slot].dd_rows;
  if (items) *items = ctx->slot[slot].dd_items;
  return LCV_OK;
}

int lcv_debug_dedup_hash_bits(lcv_ctx* ctx, int bits) {
  if (!ctx || bits < 0 || bits > 64) return fail(ctx, LCV_EINVAL, "lcv_debug_dedup_hash_bits: 0 <= bits <= 64");
  ctx->dedup_hash_bits = (uint32_t)bits;
  return LCV_OK;
}

int lcv_set_config(lcv_ctx* ctx, uint64_t slots_per_epoch, uint64_t epochs_per_sync_committee_period,
                   const uint64_t* fork_epochs4, const uint8_t* fork_versions20, const uint8_t* domain_sync_committee4) {
  if (!ctx || !fork_epochs4 || !fork_versions20 || !domain_sync_committee4) return LCV_EINVAL;
  if (slots_per_epoch == 0 || epochs_per_sync_committee_period == 0 ||
      slots_per_epoch > (UINT64_MAX >> 1) / epochs_per_sync_committee_period)
    return fail(ctx, LCV_EINVAL, "lcv_set_config: slots_per_epoch and epochs_per_sync_committee_period must be >= 1");
  for (int k = 1; k < 4; ++k)
    if (fork_epochs4[k] < fork_epochs4[k - 1])
      return fail(ctx, LCV_EINVAL, "lcv_set_config: fork epochs must be non-decreasing (altair <= bellatrix <= capella <= deneb)");
  NetConfig c;
  c.slots_per_epoch = slots_per_epoch;
  c.epochs_per_period = epochs_per_sync_committee_period;
  for (int k = 0; k < 4; ++k) c.fork_epoch[k] = fork_epochs4[k];
  for (int k = 0; k < 5; ++k) c.fork_version[k] = host_be32(fork_versions20 + 4 * k);
  c.domain_sync_committee = host_be32(domain_sync_committee4);
  ctx->cfg = c;
  return LCV_OK;
}

int lcv_last_timings(lcv_ctx* ctx, float* ms_out, int max_stages, int* nstages) {
  if (!ctx) return LCV_EINVAL;
  const int k = max_stages < ST_COUNT ? max_stages : ST_COUNT;
  for (int s = 0; s < k; ++s) ms_out[s] = ctx->stage_ms[s];
  if (nstages) *nstages = ST_COUNT;
  return LCV_OK;
}

// ---- FastAggregateVerify
// agg_items (> n only for one FastAggregateVerify call over > 512 keys, n == 1): rows of cid / bits
// describe agg_items 512-key slices whose aggregates are summed into item 0.  Allocates host memory (the cached
// table's bytes): within the boundary (guarded)
static int fav_impl(lcv_ctx* ctx, const uint8_t* committees, uint64_t ncomm, const uint32_t* cid, const uint8_t* bits,
                    const uint8_t* msg, const uint8_t* sig, uint64_t n, uint8_t* verdict_out, uint8_t* agg_out,
                    uint8_t* agg_status_out, uint64_t agg_items = 0, uint64_t msg_len = 32) {
  if (!ctx || !committees || !cid || !bits || n == 0 || ncomm == 0) return fail(ctx, LCV_EINVAL, "fast_aggregate_verify: bad arguments");
  if (n > kChunk || agg_items > kChunk) return fail(ctx, LCV_EINVAL, "fast_aggregate_verify_batch: n > 65536 per call");
  const uint64_t rows = agg_items > n ? agg_items : n;
  for (uint64_t i = 0; i < rows; ++i)
    if (cid[i] >= ncomm) return fail(ctx, LCV_EINVAL, "fast_aggregate_verify_batch: committee id out of range");
  LCV_TRY(ensure_work(ctx, rows, 1));
  be_reset_timings(ctx);
  // the decoded, KeyValidated and summed tables of the previous call are reused when this call passes
  // byte-identical tables (the reference's usage: one committee signs a whole period's updates)
  const size_t table_bytes = ncomm * 512 * 48;
  const bool cached = ctx->adhoc.raw.p && ctx->adhoc.ncomm == ncomm && ctx->adhoc_src.size() == table_bytes &&
                      memcmp(ctx->adhoc_src.data(), committees, table_bytes) == 0;
  if (!cached) {
    ctx->adhoc_src.clear();
    LCV_TRY(ensure_committees(ctx, ctx->adhoc, ncomm, 512 * 48));
    LCV_TRY(be_h2d(ctx, ctx->adhoc.raw.p, committees, table_bytes));
    LCV_TRY(build_committees(ctx, ctx->adhoc));
    ctx->adhoc_src.assign(committees, committees + table_bytes);
  }
  CommitteeDev C = committee_view(ctx->adhoc, nullptr);
  Scratch mtmp(ctx), tmp(ctx);  // mtmp: a message that is not 32 bytes (n == 1): its bytes, hashed into b0 on device
  LCV_TRY(tmp.alloc(rows * (K_BITS + K_SIG + 32)));
  uint8_t* t = tmp.p;
  int rc = be_h2d(ctx, t, bits, K_BITS * rows);
  if (rc == LCV_OK && sig) rc = be_h2d(ctx, t + K_BITS * rows, sig, K_SIG * n);
  if (rc == LCV_OK && msg && msg_len != 32) {
    rc = mtmp.alloc(msg_len ? msg_len : 1);
    if (rc == LCV_OK) rc = be_h2d(ctx, mtmp.p, msg, msg_len);
  } else if (rc == LCV_OK && msg) {
    rc = be_h2d(ctx, t + (K_BITS + K_SIG) * rows, msg, 32 * n);
  }
  if (rc == LCV_OK) rc = be_h2d(ctx, ctx->W.comm_id, cid, 4 * rows);
  if (rc == LCV_OK) rc = be_memset(ctx, ctx->W.pre_reason, 0, rows);
  BatchDev B;
  memset(&B, 0, sizeof(B));
  B.bits = t;
  B.sig = t + 64 * rows;
  B.n = (uint32_t)n;
  if (rc == LCV_OK && verdict_out) {
    if (mtmp.p) {
      rc = be_launch(ctx, F_msg_import_b0{mtmp.p, msg_len, ctx->W}, 1);
      ctx->W.msg_b0 = 1;
    } else {
      rc = be_launch(ctx, F_msg_import{t + (K_BITS + K_SIG) * rows, ctx->W}, (uint32_t)n);
    }
    if (rc == LCV_OK) rc = run_bls(ctx, B, C, (uint32_t)n, (uint32_t)agg_items);
    ctx->W.msg_b0 = 0;
    if (rc == LCV_OK) rc = be_d2h(ctx, verdict_out, ctx->W.verdict, n);
  } else if (rc == LCV_OK) {  // aggregate only
    rc = be_launch_team(ctx, F_agg_team{B, C, ctx->W}, (uint32_t)n);
    if (rc == LCV_OK) rc = be_launch(ctx, F_export_g1{ctx->W.pk, ctx->W.cap, t + 64 * rows}, (uint32_t)n);
    if (rc == LCV_OK) rc = be_d2h(ctx, agg_out, t + 64 * rows, 96 * n);
    if (rc == LCV_OK) rc = be_d2h(ctx, agg_status_out, ctx->W.agg_status, n);
  }
  if (rc == LCV_OK) rc = be_sync(ctx);
  tmp.release();
  mtmp.release();
  be_collect_timings(ctx);
  return rc;
}

int lcv_fast_aggregate_verify_batch(lcv_ctx* ctx, const uint8_t* committees, uint64_t ncomm, const uint32_t* cid,
                                    const uint8_t* bits64, const uint8_t* msg32, const uint8_t* sig96, uint64_t n,
                                    uint8_t* verdict_out) {
  if (!msg32 || !sig96 || !verdict_out) return fail(ctx, LCV_EINVAL, "fast_aggregate_verify_batch: null argument");
  return guarded(ctx, "fast_aggregate_verify_batch", [&] {
    return fav_impl(ctx, committees, ncomm, cid, bits64, msg32, sig96, n, verdict_out, nullptr, nullptr);
  });
}

int lcv_fast_aggregate_verify(lcv_ctx* ctx, const uint8_t* pks, uint64_t npk, const uint8_t* msg, uint64_t msg_len,
                              const uint8_t* sig96, int* result) {
  if (!ctx || !result || (!msg && msg_len) || !sig96 || (npk && !pks))
    return fail(ctx, LCV_EINVAL, "fast_aggregate_verify: null argument");
  static const uint8_t kEmpty[1] = {0};
  const uint8_t* msg32 = msg ? msg : kEmpty;
  *result = 0;
  if (npk == 0) return LCV_OK;  // FastAggregateVerify([]) is False
  // the keys fill ceil(npk / 512) committee tables (zero padding, never selected); slice k's bits
  // select its keys, and the slices' aggregates are summed on the device (item_agg_fold)
  const uint64_t m = (npk + 511) / 512;
  if (m > kChunk) return fail(ctx, LCV_EINVAL, "fast_aggregate_verify: too many pubkeys");
  return guarded(ctx, "fast_aggregate_verify", [&]() -> int {
    std::vector<uint8_t> table(m * 512 * 48, 0), bits(m * 64, 0);
    std::vector<uint32_t> cid(m);
    memcpy(table.data(), pks, npk * 48);
    for (uint64_t j = 0; j < npk; ++j) bits[j / 8] |= (uint8_t)(1u << (j % 8));
    for (uint64_t k = 0; k < m; ++k) cid[k] = (uint32_t)k;
    uint8_t v = 0;
    LCV_TRY(fav_impl(ctx, table.data(), m, cid.data(), bits.data(), msg32, sig96, 1, &v, nullptr, nullptr, m > 1 ? m : 0,
                     msg_len));
    *result = v ? 1 : 0;
    return LCV_OK;
  });
}

int lcv_debug_aggregate(lcv_ctx* ctx, const uint8_t* committees, uint64_t ncomm, const uint32_t* cid,
                        const uint8_t* bits64, uint64_t n, uint8_t* out96, uint8_t* status) {
  if (!out96 || !status) return fail(ctx, LCV_EINVAL, "debug_aggregate: null argument");
  return guarded(ctx, "debug_aggregate", [&] {
    return fav_impl(ctx, committees, ncomm, cid, bits64, nullptr, nullptr, n, nullptr, out96, status);
  });
}

}  // extern "C"

// ---- generic "bytes in -> kernel -> bytes out" helper
// (the boundary: the offsets and pointers are host vectors)
typedef std::initializer_list<std::pair<const void*, size_t>> SimpleIns;
typedef std::initializer_list<std::pair<void*, size_t>> SimpleOuts;
template <class MakeF> static int simple_call(lcv_ctx* ctx, uint64_t n, SimpleIns ins, SimpleOuts outs, MakeF make) {
  if (!ctx) return LCV_EINVAL;
  if (n == 0) return LCV_OK;
  if (n > 0xffffffffull) return fail(ctx, LCV_EINVAL, "n too large");
  return guarded(ctx, "simple_call", [&]() -> int {
    Layout l;
    std::vector<size_t> offs;
    for (auto& p : ins) offs.push_back(l.take(p.second));
    for (auto& p : outs) offs.push_back(l.take(p.second));
    Scratch mem(ctx);
    LCV_TRY(mem.alloc(l.total() ? l.total() : 256));
    std::vector<uint8_t*> dptr;
    for (size_t off : offs) dptr.push_back(mem.p + off);
    size_t k = 0;
    for (auto& p : ins) LCV_TRY(be_h2d(ctx, dptr[k++], p.first, p.second));
    LCV_TRY(make(dptr));
    for (auto& p : outs) LCV_TRY(be_d2h(ctx, p.first, dptr[k++], p.second));
    return be_sync(ctx);  // (then the scratch's free)
  });
}

extern "C" {

int lcv_merkle_branch_batch(lcv_ctx* ctx, const uint8_t* leaf32, const uint8_t* branch, uint32_t depth, uint64_t index,
                            const uint8_t* root32, uint64_t n, uint8_t* out) {
  if (!ctx || !leaf32 || !root32 || !out || (depth && !branch) || depth > 64) return fail(ctx, LCV_EINVAL, "merkle: bad arguments");
  static const uint8_t dummy[32] = {};
  const uint8_t* br = depth ? branch : dummy;
  const size_t brb = depth ? (size_t)32 * depth * n : 32;
  return simple_call(ctx, n, {{leaf32, 32 * n}, {br, brb}, {root32, 32 * n}}, {{out, n}}, [&](std::vector<uint8_t*>& d) {
    return be_launch(ctx, F_merkle{d[0], d[1], d[2], d[3], depth, index}, (uint32_t)n);
  });
}

int lcv_htr_sync_committee_batch(lcv_ctx* ctx, const uint8_t* committees, uint64_t n, uint8_t* roots) {
  if (!ctx || !committees || !roots) return fail(ctx, LCV_EINVAL, "htr_sync_committee: null argument");
  return simple_call(ctx, n, {{committees, (size_t)K_SC * n}}, {{roots, 32 * n}}, [&](std::vector<uint8_t*>& d) {
    return be_launch(ctx, F_htr_sc{d[0], d[1]}, (uint32_t)n);
  });
}

int lcv_bootstrap_check_batch(lcv_ctx* ctx, const uint8_t* beacon112, const uint8_t* exec832,
                              const uint8_t* exec_branch128, const uint8_t* committees, const uint8_t* committee_branch160,
                              const uint8_t* trusted_root32, uint64_t n, uint8_t* reason_out) {
  if (!ctx || !beacon112 || !exec832 || !exec_branch128 || !committees || !committee_branch160 || !trusted_root32 ||
      !reason_out)
    return fail(ctx, LCV_EINVAL, "bootstrap: null argument");
  return simple_call(ctx, n,
                     {{beacon112, (size_t)K_BEACON * n}, {exec832, (size_t)K_EXEC * n},
                      {exec_branch128, (size_t)K_EXEC_BRANCH * n}, {committees, (size_t)K_SC * n},
                      {committee_branch160, (size_t)K_NSC_BRANCH * n}, {trusted_root32, 32 * n}},
                     {{reason_out, n}}, [&](std::vector<uint8_t*>& d) {
                       return be_launch(ctx, F_bootstrap{d[0], d[1], d[2], d[3], d[4], d[5], d[6], ctx->cfg}, (uint32_t)n);
                     });
}

int lcv_sk_to_pk_batch(lcv_ctx* ctx, const uint8_t* sk32, uint64_t n, uint8_t* pk48) {
  if (!ctx || !sk32 || !pk48) return fail(ctx, LCV_EINVAL, "sk_to_pk: null argument");
  return simple_call(ctx, n, {{sk32, 32 * n}}, {{pk48, 48 * n}}, [&](std::vector<uint8_t*>& d) {
    return be_launch(ctx, F_sk_to_pk{d[0], d[1]}, (uint32_t)n);
  });
}

int lcv_sign_batch(lcv_ctx* ctx, const uint8_t* sk32, const uint8_t* msg32, uint64_t n, uint8_t* sig96) {
  if (!ctx || !sk32 || !msg32 || !sig96) return fail(ctx, LCV_EINVAL, "sign: null argument");
  return simple_call(ctx, n, {{sk32, 32 * n}, {msg32, 32 * n}}, {{sig96, 96 * n}}, [&](std::vector<uint8_t*>& d) {
    return be_launch(ctx, F_sign{d[0], d[1], d[2]}, (uint32_t)n);
  });
}

int lcv_debug_fp(lcv_ctx* ctx, const uint8_t* a48, const uint8_t* b48, uint64_t n, uint8_t* out288, uint8_t* ok) {
  if (!ctx || !a48 || !b48 || !out288 || !ok) return fail(ctx, LCV_EINVAL, "debug_fp: null argument");
  return simple_call(ctx, n, {{a48, 48 * n}, {b48, 48 * n}}, {{out288, 288 * n}, {ok, n}}, [&](std::vector<uint8_t*>& d) {
    return be_launch(ctx, F_dbg_fp{d[0], d[1], d[2], d[3]}, (uint32_t)n);
  });
}

int lcv_debug_fp_pow(lcv_ctx* ctx, const uint8_t* a48, uint64_t n, uint8_t* out96) {
  if (!ctx || !a48 || !out96) return fail(ctx, LCV_EINVAL, "debug_fp_pow: null argument");
  return simple_call(ctx, n, {{a48, 48 * n}}, {{out96, 96 * n}}, [&](std::vector<uint8_t*>& d) {
    if (fan_on(ctx, n)) return be_launch(ctx, F_dbg_pow_lat{{d[0], d[1]}}, (uint32_t)n);
    return be_launch(ctx, F_dbg_pow{d[0], d[1]}, (uint32_t)n);
  });
}

int lcv_debug_hash_to_g2(lcv_ctx* ctx, const uint8_t* msg32, uint64_t n, uint8_t* out192, uint8_t* inf) {
  if (!ctx || !msg32 || !out192 || !inf) return fail(ctx, LCV_EINVAL, "debug_hash_to_g2: null argument");
  if (n > kChunk) return fail(ctx, LCV_EINVAL, "debug_hash_to_g2: n > 65536");
  LCV_TRY(ensure_work(ctx, n, 1));
  return simple_call(ctx, n, {{msg32, 32 * n}}, {{out192, 4 * 48 * n}, {inf, n}}, [&](std::vector<uint8_t*>& d) {
    Work W = ctx->W;
    LCV_TRY(be_launch(ctx, F_msg_import{d[0], W}, (uint32_t)n));
    LCV_TRY(hash_to_g2_stage(ctx, ctx->W, (uint32_t)n));
    LCV_TRY(be_launch(ctx, F_export_g2{W.qh, W.cap, d[1]}, (uint32_t)n));
    return be_d2d(ctx, d[2], W.qh_inf, n);
  });
}

int lcv_debug_g2_decompress(lcv_ctx* ctx, const uint8_t* sig96, uint64_t n, uint8_t* out192, uint8_t* status) {
  if (!ctx || !sig96 || !out192 || !status) return fail(ctx, LCV_EINVAL, "debug_g2_decompress: null argument");
  if (n > kChunk) return fail(ctx, LCV_EINVAL, "debug_g2_decompress: n > 65536");
  LCV_TRY(ensure_work(ctx, n, 1));
  return simple_call(ctx, n, {{sig96, K_SIG * n}}, {{out192, 4 * 48 * n}, {status, n}}, [&](std::vector<uint8_t*>& d) {
    Work W = ctx->W;
    BatchDev B;
    memset(&B, 0, sizeof(B));
    B.sig = d[0];
    B.n = (uint32_t)n;
    LCV_TRY(sig_decode_check(ctx, B, ctx->W, (uint32_t)n));
    LCV_TRY(be_launch(ctx, F_export_g2{W.qs, W.cap, d[1]}, (uint32_t)n));
    return be_d2d(ctx, d[2], W.sig_status, n);
  });
}

int lcv_debug_pairing(lcv_ctx* ctx, const uint8_t* p96, const uint8_t* q192, uint64_t n, uint8_t* out576) {
  if (!ctx || !p96 || !q192 || !out576) return fail(ctx, LCV_EINVAL, "debug_pairing: null argument");
  if (n > kChunk) return fail(ctx, LCV_EINVAL, "debug_pairing: n > 65536");
  LCV_TRY(ensure_work(ctx, n, 1));
  be_reset_timings(ctx);
  const int rc = simple_call(ctx, n, {{p96, 96 * n}, {q192, 4 * 48 * n}}, {{out576, 576 * n}}, [&](std::vector<uint8_t*>& d) {
    Work W = ctx->W;
    LCV_TRY(be_launch(ctx, F_import_pq{d[0], d[1], W}, (uint32_t)n));
    LCV_TRY(pairing_check(ctx, ctx->W, (uint32_t)n));
    return be_launch(ctx, F_export_fp12{W.f, W.cap, d[2]}, (uint32_t)n);
  });
  be_collect_timings(ctx);  // miller / final_exp kernel times (lcv_last_timings)
  return rc;
}

// ---- test hooks of randomised batch verification (lcv_rlc.hpp)
int lcv_debug_rlc_coeffs(lcv_ctx* ctx, uint64_t counter, uint64_t n, uint64_t* out_u64) {
  if (!ctx || !out_u64) return fail(ctx, LCV_EINVAL, "lcv_debug_rlc_coeffs: null argument");
  if (!ctx->rlc_seeded) return fail(ctx, LCV_ESTATE, "lcv_debug_rlc_coeffs: lcv_set_rlc has set no seed");
  RlcKey key;
  for (int k = 0; k < 8; ++k) key.seed[k] = ctx->rlc_seed[k];
  key.counter = counter;
  return simple_call(ctx, n, {}, {{out_u64, 8 * n}}, [&](std::vector<uint8_t*>& d) {
    return be_launch(ctx, F_dbg_rlc_coeffs{key, (uint64_t*)d[0]}, (uint32_t)n);
  });
}

int lcv_debug_rlc_scale(lcv_ctx* ctx, const uint8_t* p96, const uint64_t* r_u64, uint64_t n, uint8_t* out96) {
  if (!ctx || !p96 || !r_u64 || !out96) return fail(ctx, LCV_EINVAL, "lcv_debug_rlc_scale: null argument");
  return simple_call(ctx, n, {{p96, 96 * n}, {r_u64, 8 * n}}, {{out96, 96 * n}}, [&](std::vector<uint8_t*>& d) {
    return be_launch(ctx, F_dbg_rlc_scale{d[0], (const uint64_t*)d[1], d[2]}, (uint32_t)n);
  });
}

}  // extern "C"

// ------------------------------------------------------------------ the producer side (lcv_producer.hpp)
// One device allocation per call: the view tables, the cases, the stage-0 / stage-1 scratch rows, the reasons (and
// what a caller adds: `extra`).  Every index a kernel follows is checked on the host before anything is launched.
struct ProdRun {
  Scratch mem;
  explicit ProdRun(lcv_ctx* ctx) : mem(ctx) {}
  uint8_t* extra = nullptr;  // the caller's part of the allocation
  uint8_t* reason = nullptr; // [n]
  ProdStates S; ProdBlocks K; ProdCases C; ProdScratch X;
  const uint32_t* idx0 = nullptr;  // the bootstrap entry's two index columns
  const uint32_t* idx1 = nullptr;
};

static int prod_check_views(lcv_ctx* ctx, const char* who, const lcv_state_views* s, uint64_t ns, const lcv_block_views* b,
                            uint64_t nb, const uint8_t* committees, uint64_t ncomm) {
  const std::string w(who);
  if (!s->slot || !s->latest_block_header || !s->fin_epoch || !s->fin_root || !s->field_roots || !s->cur_index ||
      !s->nxt_index || !b->slot || !b->proposer_index || !b->parent_root || !b->state_root || !b->bits || !b->signature ||
      !b->execution || !b->exec_kind || !b->body_roots || !committees)
    return fail(ctx, LCV_EINVAL, w + ": null column");
  if (ns == 0 || nb == 0 || ncomm == 0 || ns >= 0xffffffffull || nb >= 0xffffffffull || ncomm >= 0xffffffffull)
    return fail(ctx, LCV_EINVAL, w + ": need 0 < ns, nb, ncomm < 2^32 - 1");
  for (uint64_t t = 0; t < ns; ++t)
    if (s->cur_index[t] >= ncomm || s->nxt_index[t] >= ncomm)
      return fail(ctx, LCV_EINVAL, w + ": committee index of state view " + std::to_string(t) + " out of range");
  for (uint64_t k = 0; k < nb; ++k)
    if (b->exec_kind[k] > 2)
      return fail(ctx, LCV_EINVAL, w + ": exec_kind of block view " + std::to_string(k) + " is not 0, 1 or 2");
  return LCV_OK;
}
static int prod_check_index(lcv_ctx* ctx, const char* who, const char* col, const uint32_t* ix, uint64_t n, uint64_t lim) {
  for (uint64_t i = 0; i < n; ++i)
    if (ix[i] >= lim)
      return fail(ctx, LCV_EINVAL, std::string(who) + ": " + col + "[" + std::to_string(i) + "] = " +
                                       std::to_string(ix[i]) + " out of range (" + std::to_string(lim) + " rows)");
  return LCV_OK;
}

// uploads the views (and the n-row index columns ix[0 .. nix), 4 bytes per entry), hashes the committee rows of
// `pool` (device, ncomm rows of K_SC bytes; null: `committees` is uploaded into the allocation) and runs stage 1
static int prod_views(lcv_ctx* ctx, const lcv_state_views* s, uint64_t ns, const lcv_block_views* b, uint64_t nb,
                      const uint8_t* committees, const uint8_t* pool, uint64_t ncomm, const void* const* ix, int nix,
                      uint64_t n, size_t extra_bytes, ProdRun& R) {
  enum { NV = 16 };
  const void* src[NV] = {s->slot, s->latest_block_header, s->fin_epoch, s->fin_root, s->field_roots, s->cur_index,
                         s->nxt_index, b->slot, b->proposer_index, b->parent_root, b->state_root, b->bits,
                         b->signature, b->execution, b->exec_kind, b->body_roots};
  const size_t bytes[NV] = {8 * ns, (size_t)K_BEACON * ns, 8 * ns, 32 * ns, 32 * PROD_STATE_FIELDS * ns, 4 * ns, 4 * ns, 8 * nb, 8 * nb,
                            32 * nb, 32 * nb, 64 * nb, 96 * nb, (size_t)K_EXEC * nb, nb, 32 * PROD_BODY_FIELDS * nb};
  Layout l;
  size_t off[NV], ixoff[8];
  for (int k = 0; k < NV; ++k) off[k] = l.take(bytes[k]);
  for (int k = 0; k < nix; ++k) ixoff[k] = l.take(4 * n);
  const size_t o_pool = l.take(pool ? 0 : (size_t)K_SC * ncomm), o_root = l.take(32 * ncomm), o_flag = l.take(ncomm);
  const size_t o_blk = l.take((size_t)PROD_BLK_ROW * nb), o_st = l.take((size_t)PROD_ST_ROW * ns);
  const size_t o_reason = l.take(n), o_extra = l.take(extra_bytes);
  LCV_TRY(R.mem.alloc(l.total()));
  uint8_t* m = R.mem.p;
  for (int k = 0; k < NV; ++k) LCV_TRY(be_h2d(ctx, m + off[k], src[k], bytes[k]));
  for (int k = 0; k < nix; ++k) LCV_TRY(be_h2d(ctx, m + ixoff[k], ix[k], 4 * n));
  if (!pool) {
    LCV_TRY(be_h2d(ctx, m + o_pool, committees, (size_t)K_SC * ncomm));
    pool = m + o_pool;
  }
  R.S = ProdStates{(const uint64_t*)(m + off[0]), m + off[1], (const uint64_t*)(m + off[2]), m + off[3], m + off[4],
                   (const uint32_t*)(m + off[5]), (const uint32_t*)(m + off[6])};
  R.K = ProdBlocks{(const uint64_t*)(m + off[7]), (const uint64_t*)(m + off[8]), m + off[9], m + off[10], m + off[11],
                   m + off[12], m + off[13], m + off[14], m + off[15]};
  if (nix == 5)
    R.C = ProdCases{(const uint32_t*)(m + ixoff[0]), (const uint32_t*)(m + ixoff[1]), (const uint32_t*)(m + ixoff[2]),
                    (const uint32_t*)(m + ixoff[3]), (const int32_t*)(m + ixoff[4])};
  if (nix == 2) { R.idx0 = (const uint32_t*)(m + ixoff[0]); R.idx1 = (const uint32_t*)(m + ixoff[1]); }
  R.X = ProdScratch{(const uint32_t*)(m + o_root), (uint32_t)ncomm, m + o_blk, m + o_st};
  R.reason = m + o_reason;
  R.extra = m + o_extra;
  // stage 0: HTR(SyncCommittee) per committee row on validation's own 64-lane tree (its store-equality flag
  // compares every row with row 0 and is not read)
  BatchDev PB = {};
  PB.nsc_pool = pool;
  PB.npool = (uint32_t)ncomm;
  CommitteeDev PC = {};
  PC.next_raw = pool;
  Work PW = Work{};
  PW.pool_cap = (uint32_t)ncomm;
  PW.nsc_root = (uint32_t*)(m + o_root);
  PW.nsc_flags = m + o_flag;
  LCV_TRY(stage(ctx, ST_PRODUCE_VIEWS, [&] { return be_launch_team(ctx, F_nsc_team{PB, PC, PW}, (uint32_t)ncomm); }));
  LCV_TRY(stage(ctx, ST_PRODUCE_VIEWS, [&] { return be_launch(ctx, F_prod_block{R.K, R.X}, (uint32_t)nb); }));
  return stage(ctx, ST_PRODUCE_VIEWS, [&] { return be_launch(ctx, F_prod_state{R.S, R.X}, (uint32_t)ns); });
}

// the producer's writable view of a batch's row columns (kBatchCols: the rows with a ProdOut member)
static ProdOut prod_out(const BatchDev& B) {
  ProdOut O = {};
  for (const ColSpec& s : kBatchCols)
    if (s.prod >= 0) slot_set(&O, s.prod, slot_get(&B, s.dev));
  return O;
}

// a resident batch's row columns (and its pool, when asked, after them) to the caller's arrays
static int prod_copy_out(lcv_ctx* ctx, const BatchDev& B, size_t n, const lcv_update_batch* out, bool with_pool,
                         size_t npool) {
  for (const ColSpec& s : kBatchCols)
    if (col_per_row(s) && s.host >= 0) LCV_TRY(be_d2h(ctx, slot_get(out, s.host), slot_get(&B, s.dev), s.width * n));
  const ColSpec& p = kBatchCols[COL_NSC_POOL];
  if (with_pool) LCV_TRY(be_d2h(ctx, slot_get(out, p.host), B.nsc_pool, p.width * npool));
  return LCV_OK;
}
static bool batch_out_null(const lcv_update_batch* o) {
  if (!o) return true;
  for (const ColSpec& s : kBatchCols)
    if (s.host >= 0 && !slot_get(o, s.host)) return true;
  return false;
}

extern "C" {

int lcv_create_updates_resident(lcv_ctx* ctx, const lcv_state_views* states, uint64_t ns, const lcv_block_views* blocks,
                                uint64_t nb, const uint8_t* committees, uint64_t ncomm, const lcv_update_cases* cases,
                                uint64_t n, int kind, uint8_t* reason_out, lcv_dbatch** out) {
  const char* who = "lcv_create_updates";
  if (out) *out = nullptr;
  if (!ctx || !states || !blocks || !committees || !cases || !reason_out || !out)
    return fail(ctx, LCV_EINVAL, std::string(who) + ": null argument");
  if (!wire_kind_ok(kind)) return fail(ctx, LCV_EINVAL, std::string(who) + ": kind is 0 (update), 1 (finality) or 2 (optimistic)");
  if (n == 0) return LCV_OK;
  if (n >= 0xffffffffull) return fail(ctx, LCV_EINVAL, std::string(who) + ": need n < 2^32 - 1");
  if (!cases->state || !cases->block || !cases->attested_state || !cases->attested_block || !cases->finalized_block)
    return fail(ctx, LCV_EINVAL, std::string(who) + ": null column");
  LCV_TRY(prod_check_views(ctx, who, states, ns, blocks, nb, committees, ncomm));
  LCV_TRY(prod_check_index(ctx, who, "state", cases->state, n, ns));
  LCV_TRY(prod_check_index(ctx, who, "block", cases->block, n, nb));
  LCV_TRY(prod_check_index(ctx, who, "attested_state", cases->attested_state, n, ns));
  LCV_TRY(prod_check_index(ctx, who, "attested_block", cases->attested_block, n, nb));
  for (uint64_t i = 0; i < n; ++i)
    if (cases->finalized_block[i] < -1 || (cases->finalized_block[i] >= 0 && (uint64_t)cases->finalized_block[i] >= nb))
      return fail(ctx, LCV_EINVAL, std::string(who) + ": finalized_block[" + std::to_string(i) + "] = " +
                                       std::to_string(cases->finalized_block[i]) + " out of range (-1, or a row of " +
                                       std::to_string(nb) + ")");
  // the batch: lcv_batch_upload's layout, the pool = the committee rows and one all-zero row
  BatchCols c;
  batch_layout(c, n, ncomm + 1, false, 0);
  NewBatch nb_(ctx);
  be_set_slot(ctx, 0);
  LCV_TRY(batch_new(ctx, c, nb_));
  lcv_dbatch* db = nb_.db;
  uint8_t* pool = db->mem.p + c.off[COL_NSC_POOL];
  ProdRun R(ctx);  // (its scratch is freed, waiting for the streams, ahead of an abandoned batch)
  be_reset_timings(ctx);
  LCV_TRY(be_h2d(ctx, pool, committees, (size_t)K_SC * ncomm));
  LCV_TRY(be_memset(ctx, pool + (size_t)K_SC * ncomm, 0, K_SC));
  const void* ix[5] = {cases->state, cases->block, cases->attested_state, cases->attested_block, cases->finalized_block};
  LCV_TRY(prod_views(ctx, states, ns, blocks, nb, committees, db->B.nsc_pool, ncomm, ix, 5, n, 0, R));
  LCV_TRY(stage(ctx, ST_PRODUCE_ROWS, [&] {
    return be_launch_team(ctx, F_prod_rows{R.S, R.K, R.C, R.X, prod_out(db->B), ctx->cfg, (uint32_t)kind,
                                           (uint32_t)ncomm, R.reason}, (uint32_t)n);
  }));
  LCV_TRY(be_d2h(ctx, reason_out, R.reason, n));
  LCV_TRY(be_sync(ctx));
  be_collect_timings(ctx);
  return nb_.hand_out(out);
}

int lcv_batch_download(lcv_ctx* ctx, lcv_dbatch* b, const uint32_t* rows, uint64_t nrows, const lcv_update_batch* out) {
  if (!ctx || !b || batch_out_null(out)) return fail(ctx, LCV_EINVAL, "lcv_batch_download: null argument");
  be_set_slot(ctx, 0);
  if (!rows) {
    LCV_TRY(prod_copy_out(ctx, b->B, b->n, out, true, b->npool));
    return be_sync(ctx);
  }
  if (nrows >= 0xffffffffull) return fail(ctx, LCV_EINVAL, "lcv_batch_download: need nrows < 2^32 - 1");
  LCV_TRY(prod_check_index(ctx, "lcv_batch_download", "rows", rows, nrows, b->n));
  LCV_TRY(be_d2h(ctx, (void*)out->nsc_pool, b->B.nsc_pool, (size_t)K_SC * b->npool));
  if (nrows == 0) return be_sync(ctx);
  // the listed rows are gathered on the device into a batch of nrows rows (no pool), which is copied out
  BatchCols c;
  batch_layout(c, nrows, 0, false, 0);
  const size_t o_rows = c.total;
  Scratch mem(ctx);
  LCV_TRY(mem.alloc(c.total + 4 * nrows));
  lcv_dbatch t;
  bind_batch(&t, mem.p, c);
  LCV_TRY(be_h2d(ctx, mem.p + o_rows, rows, 4 * nrows));
  LCV_TRY(be_launch_team(ctx, F_prod_pick{b->B, (const uint32_t*)(mem.p + o_rows), prod_out(t.B)}, (uint32_t)nrows));
  LCV_TRY(prod_copy_out(ctx, t.B, nrows, out, false, 0));
  return be_sync(ctx);
}

int lcv_create_updates(lcv_ctx* ctx, const lcv_state_views* states, uint64_t ns, const lcv_block_views* blocks,
                       uint64_t nb, const uint8_t* committees, uint64_t ncomm, const lcv_update_cases* cases,
                       uint64_t n, int kind, const lcv_update_batch* out, uint8_t* reason_out) {
  if (!ctx || batch_out_null(out)) return fail(ctx, LCV_EINVAL, "lcv_create_updates: null argument");
  lcv_dbatch* db = nullptr;
  LCV_TRY(lcv_create_updates_resident(ctx, states, ns, blocks, nb, committees, ncomm, cases, n, kind, reason_out, &db));
  if (!db) return LCV_OK;  // n == 0
  const int rc = lcv_batch_download(ctx, db, nullptr, 0, out);
  lcv_batch_free(ctx, db);
  return rc;
}

// lcv_rank_updates over a resident batch: F_rank on the batch where it lies, the records copied out
int lcv_rank_resident(lcv_ctx* ctx, lcv_dbatch* b, uint8_t* rank_out) {
  if (!ctx || !b || !rank_out) return fail(ctx, LCV_EINVAL, "lcv_rank_resident: null argument");
  if (b->n == 0) return LCV_OK;
  Scratch mem(ctx);
  be_set_slot(ctx, 0);
  LCV_TRY(mem.alloc(rank_index(b->n)));
  Work W = Work{};
  W.rank = mem.p;
  Params P = {};
  P.cfg = ctx->cfg;
  be_reset_timings(ctx);
  LCV_TRY(rank_stage(ctx, b->B, P, W, (uint32_t)b->n));
  LCV_TRY(be_d2h(ctx, rank_out, W.rank, rank_index(b->n)));
  LCV_TRY(be_sync(ctx));
  be_collect_timings(ctx);
  return LCV_OK;
}

int lcv_create_bootstraps(lcv_ctx* ctx, const lcv_state_views* states, uint64_t ns, const lcv_block_views* blocks,
                          uint64_t nb, const uint8_t* committees, uint64_t ncomm, const uint32_t* state_idx,
                          const uint32_t* block_idx, uint64_t n, uint8_t* beacon112, uint8_t* exec832,
                          uint8_t* exec_branch128, uint32_t* committee_index, uint8_t* committee_branch160,
                          uint8_t* reason_out) {
  const char* who = "lcv_create_bootstraps";
  if (!ctx || !states || !blocks || !committees || !state_idx || !block_idx || !beacon112 || !exec832 || !exec_branch128 ||
      !committee_index || !committee_branch160 || !reason_out)
    return fail(ctx, LCV_EINVAL, std::string(who) + ": null argument");
  if (n == 0) return LCV_OK;
  if (n >= 0xffffffffull) return fail(ctx, LCV_EINVAL, std::string(who) + ": need n < 2^32 - 1");
  LCV_TRY(prod_check_views(ctx, who, states, ns, blocks, nb, committees, ncomm));
  LCV_TRY(prod_check_index(ctx, who, "state_idx", state_idx, n, ns));
  LCV_TRY(prod_check_index(ctx, who, "block_idx", block_idx, n, nb));
  const size_t width[5] = {K_BEACON, K_EXEC, K_EXEC_BRANCH, 4, K_NSC_BRANCH};
  size_t off[5];
  Layout extra;
  for (int k = 0; k < 5; ++k) off[k] = extra.take(width[k] * n);
  ProdRun R(ctx);
  be_set_slot(ctx, 0);
  be_reset_timings(ctx);
  const void* ix[2] = {state_idx, block_idx};
  LCV_TRY(prod_views(ctx, states, ns, blocks, nb, committees, nullptr, ncomm, ix, 2, n, extra.total(), R));
  uint8_t* e = R.extra;
  const ProdBootOut O = {e + off[0], e + off[1], e + off[2], (uint32_t*)(e + off[3]), e + off[4], R.reason};
  LCV_TRY(stage(ctx, ST_PRODUCE_ROWS, [&] {
    return be_launch_team(ctx, F_prod_boot{R.S, R.K, R.idx0, R.idx1, R.X, O, ctx->cfg, (uint32_t)ncomm}, (uint32_t)n);
  }));
  void* dst[5] = {beacon112, exec832, exec_branch128, committee_index, committee_branch160};
  for (int k = 0; k < 5; ++k) LCV_TRY(be_d2h(ctx, dst[k], e + off[k], width[k] * n));
  LCV_TRY(be_d2h(ctx, reason_out, R.reason, n));
  LCV_TRY(be_sync(ctx));
  be_collect_timings(ctx);
  return LCV_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ SSZ wire bytes of a resident batch (lcv_wire_enc.hpp)
// The message areas are written into device scratch one chunk at a time and copied out before the scratch is reused:
// at most LCV_ENCODE_SCRATCH_BYTES of areas, whatever the number of rows.  Copies and launches share one stream, so
// a chunk's kernel starts after the previous chunk's areas have left.
static_assert(LCV_ENCODE_SCRATCH_BYTES >= wire_encode_pitch(WIRE_UPDATE), "the scratch holds one message");

extern "C" {

uint64_t lcv_encode_pitch(int kind) { return wire_kind_ok(kind) ? wire_encode_pitch((uint32_t)kind) : 0; }

int lcv_debug_set_encode_chunk(lcv_ctx* ctx, uint64_t rows) {
  if (!ctx) return LCV_EINVAL;
  ctx->enc_chunk = rows;  // 0: as many as fit the scratch bound
  return LCV_OK;
}

int lcv_batch_encode(lcv_ctx* ctx, lcv_dbatch* b, const uint32_t* rows, uint64_t nrows, int kind, int fork,
                     uint8_t* out, uint32_t* len_out, uint8_t* fork_out, uint8_t* version_out, uint8_t* status_out) {
  const char* who = "lcv_batch_encode";
  if (!ctx || !b || !out || !len_out || !fork_out || !version_out || !status_out)
    return fail(ctx, LCV_EINVAL, std::string(who) + ": null argument");
  if (!wire_kind_ok(kind)) return fail(ctx, LCV_EINVAL, std::string(who) + ": kind is 0 (update), 1 (finality) or 2 (optimistic)");
  if (fork != LCV_FORK_AUTO && !wire_fork_ok(fork))
    return fail(ctx, LCV_EINVAL, std::string(who) + ": fork is 0 (Deneb), 1 (Capella), 2 (Altair) or LCV_FORK_AUTO");
  if (rows) {
    if (nrows >= 0xffffffffull) return fail(ctx, LCV_EINVAL, std::string(who) + ": need nrows < 2^32 - 1");
    LCV_TRY(prod_check_index(ctx, who, "rows", rows, nrows, b->n));
  }
  const uint64_t m = rows ? nrows : b->n;
  if (m == 0) return LCV_OK;
  const uint64_t pitch = wire_encode_pitch((uint32_t)kind);
  uint64_t chunk = LCV_ENCODE_SCRATCH_BYTES / pitch;
  if (ctx->enc_chunk && ctx->enc_chunk < chunk) chunk = ctx->enc_chunk;
  if (m < chunk) chunk = m;
  Layout l;
  const size_t o_area = l.take(chunk * pitch), o_meta = l.take(chunk * ENC_META_BYTES), o_rows = l.take(4 * chunk);
  return guarded(ctx, who, [&]() -> int {
    std::vector<uint8_t> meta(m * ENC_META_BYTES);
    be_set_slot(ctx, 0);
    LCV_TRY(ctx->enc_mem.grow(ctx, l.total()));
    uint8_t* d = ctx->enc_mem.p;
    be_reset_timings(ctx);
    for (uint64_t c0 = 0; c0 < m; c0 += chunk) {
      const uint64_t mc = std::min(chunk, m - c0);
      if (rows) LCV_TRY(be_h2d(ctx, d + o_rows, rows + c0, 4 * mc));
      const EncArgs A = {b->B, rows ? (const uint32_t*)(d + o_rows) : nullptr, (uint32_t)c0, d + o_area, d + o_meta, ctx->cfg,
                         (uint32_t)kind, (int32_t)fork, (uint32_t)pitch};
      LCV_TRY(stage(ctx, ST_WIRE_ENCODE, [&] { return be_launch_team(ctx, F_wire_enc{A}, (uint32_t)mc); }));
      LCV_TRY(be_d2h(ctx, out + c0 * pitch, d + o_area, mc * pitch));
      LCV_TRY(be_d2h(ctx, meta.data() + c0 * ENC_META_BYTES, d + o_meta, mc * ENC_META_BYTES));
    }
    LCV_TRY(be_sync(ctx));
    be_collect_timings(ctx);
    for (uint64_t i = 0; i < m; ++i) {
      const uint8_t* r = meta.data() + i * ENC_META_BYTES;
      memcpy(&len_out[i], r, 4);
      fork_out[i] = r[4];
      status_out[i] = r[5];
      memcpy(version_out + 4 * i, r + 8, 4);
    }
    return LCV_OK;
  });
}

int lcv_encode_updates(lcv_ctx* ctx, const lcv_update_batch* batch, int kind, int fork, uint8_t* out, uint32_t* len_out,
                       uint8_t* fork_out, uint8_t* version_out, uint8_t* status_out) {
  const char* who = "lcv_encode_updates";
  if (!ctx || !batch || !out || !len_out || !fork_out || !version_out || !status_out)
    return fail(ctx, LCV_EINVAL, std::string(who) + ": null argument");
  if (!wire_kind_ok(kind)) return fail(ctx, LCV_EINVAL, std::string(who) + ": kind is 0 (update), 1 (finality) or 2 (optimistic)");
  if (fork != LCV_FORK_AUTO && !wire_fork_ok(fork))
    return fail(ctx, LCV_EINVAL, std::string(who) + ": fork is 0 (Deneb), 1 (Capella), 2 (Altair) or LCV_FORK_AUTO");
  if (batch->n == 0) return LCV_OK;
  lcv_dbatch* db = nullptr;
  LCV_TRY(batch_upload(ctx, batch, nullptr, &db));
  const int rc = lcv_batch_encode(ctx, db, nullptr, 0, kind, fork, out, len_out, fork_out, version_out, status_out);
  lcv_batch_free(ctx, db);
  return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ SSZ wire messages into a resident batch (lcv_wire_dec.hpp)
// The messages go through the context's pinned buffer — message i at a 16-byte aligned offset, 16 zero bytes behind
// the last, then the (offset, length, fork) of every message — and ONE DMA into the context's device scratch, which
// also holds the rows' records and the lists of the pool resolution.  Updates (kind 0) take two passes of F_wire_dec:
// the plan and the committee hashes first, because the batch's layout depends on the number of pool rows; then, with
// the batch allocated, the rows.  The other kinds have one pool row, SyncCommittee(), and take the second pass only.
struct DecScratch { size_t meta, stage_bytes, rec, pairs, differ, pool_src, total; };
static DecScratch dec_scratch(size_t msg_bytes, size_t n) {
  Layout l;
  DecScratch s;
  l.take(msg_bytes);  // the messages, at offset 0
  s.meta = l.take(n * DEC_META_BYTES);
  s.stage_bytes = s.meta + n * DEC_META_BYTES;  // what the one DMA moves
  s.rec = l.take(n * DEC_REC_BYTES);
  s.pairs = l.take(n * DEC_PAIR_BYTES);
  s.differ = l.take(4 * n);
  s.pool_src = l.take(8 * (n + 1));
  s.total = l.total();
  return s;
}

// The distinct committees of the rows `cand` (ascending; valid updates whose committee is not all zero): rep[i] = the
// first row whose committee equals row i's.  The rows are grouped by their (truncated) hash alone; then every row but
// a group's first is compared in full with its tentative representative on the device (F_sc_confirm), the rows that
// differ form the next candidate group under their lowest row, and the compare repeats: one launch per extra distinct
// content under one hash value, none at 64 bits in practice (the loop: dedup_confirm_groups, which lcv_batch_classify
// shares).  coff[i]: the scratch offset of row i's committee
static int dec_resolve_pool(lcv_ctx* ctx, uint8_t* d, const DecScratch& S, const std::vector<uint32_t>& cand,
                            const uint8_t* rec, const std::vector<uint64_t>& coff, std::vector<uint32_t>& rep) {
  auto hash_of = [&](uint32_t row) {
    uint64_t h;
    memcpy(&h, rec + (size_t)DEC_REC_BYTES * row + 8, 8);
    return h;
  };
  dedup_group(
      (uint32_t)cand.size(), ctx->dec_hash_bits, ctx->dec_table, [&](uint32_t j) { return hash_of(cand[j]); },
      [](uint32_t, uint32_t) { return true; }, [&](uint32_t j) { rep[cand[j]] = cand[j]; },
      [&](uint32_t a, uint32_t j) { rep[cand[j]] = cand[a]; });
  std::vector<uint32_t> pending;
  std::vector<uint64_t> pairs;
  for (uint32_t r : cand)
    if (rep[r] != r) pending.push_back(r);
  return dedup_confirm_groups(rep, pending, [&](const std::vector<uint32_t>& pend, const std::vector<uint32_t>& rp,
                                                std::vector<uint32_t>& differ) -> int {
    const size_t m = pend.size();
    pairs.resize(2 * m);
    for (size_t k = 0; k < m; ++k) {
      pairs[2 * k] = coff[pend[k]];
      pairs[2 * k + 1] = coff[rp[pend[k]]];
    }
    LCV_TRY(be_h2d(ctx, d + S.pairs, pairs.data(), DEC_PAIR_BYTES * m));
    const ScConfirmArgs A = {d, d + S.pairs, (uint32_t*)(d + S.differ)};
    LCV_TRY(stage(ctx, ST_DECODE_POOL, [&] { return be_launch_team(ctx, F_sc_confirm{A}, (uint32_t)m); }));
    LCV_TRY(be_d2h(ctx, differ.data(), d + S.differ, 4 * m));
    return be_sync(ctx);
  });
}

extern "C" {

int lcv_debug_decode_hash_bits(lcv_ctx* ctx, uint32_t bits) {
  if (!ctx || bits > 64) return fail(ctx, LCV_EINVAL, "lcv_debug_decode_hash_bits: bits <= 64");
  ctx->dec_hash_bits = bits;
  return LCV_OK;
}

int lcv_last_decode_timings(lcv_ctx* ctx, float ms_out[2]) {
  if (!ctx || !ms_out) return fail(ctx, LCV_EINVAL, "lcv_last_decode_timings: null argument");
  ms_out[0] = ctx->stage_ms[ST_WIRE_DECODE];
  ms_out[1] = ctx->stage_ms[ST_DECODE_POOL];
  return LCV_OK;
}

int lcv_batch_decode(lcv_ctx* ctx, const uint8_t* buf, uint64_t buf_len, const uint64_t* offsets, const uint64_t* lengths,
                     uint64_t n, int kind, int fork, const uint8_t* forks, uint8_t* status_out, lcv_dbatch** out) {
  const std::string who = "lcv_batch_decode";
  if (out) *out = nullptr;
  if (!ctx || !buf || !offsets || !lengths || !status_out || !out) return fail(ctx, LCV_EINVAL, who + ": null argument");
  if (!wire_kind_ok(kind)) return fail(ctx, LCV_EINVAL, who + ": kind is 0 (update), 1 (finality) or 2 (optimistic)");
  if (!forks && !wire_fork_ok(fork)) return fail(ctx, LCV_EINVAL, who + ": fork is 0 (Deneb), 1 (Capella) or 2 (Altair)");
  if (n > LCV_DECODE_MAX_ROWS)
    return fail(ctx, LCV_EINVAL, who + ": n = " + std::to_string(n) + " above LCV_DECODE_MAX_ROWS");
  uint64_t msg_bytes = 16;  // the zero padding behind the last message
  for (uint64_t i = 0; i < n; ++i) {
    if (lengths[i] > buf_len || offsets[i] > buf_len - lengths[i])
      return fail(ctx, LCV_EINVAL, who + ": message " + std::to_string(i) + ": offsets + lengths = " + std::to_string(offsets[i]) +
                                       " + " + std::to_string(lengths[i]) + " is past buf_len " + std::to_string(buf_len));
    if (lengths[i] <= LCV_DECODE_MAX_BYTES) msg_bytes += (lengths[i] + 15) & ~(uint64_t)15;
    if (lengths[i] > LCV_DECODE_MAX_BYTES || msg_bytes > LCV_DECODE_MAX_BYTES)
      return fail(ctx, LCV_EINVAL, who + ": staged bytes above LCV_DECODE_MAX_BYTES at message " + std::to_string(i));
  }
  if (n == 0) return LCV_OK;
  return guarded(ctx, who.c_str(), [&]() -> int {
    const DecScratch S = dec_scratch((size_t)msg_bytes, (size_t)n);
    std::vector<uint8_t> rec(n * DEC_REC_BYTES);
    std::vector<uint32_t> nsc_index(n, 0u), rep, cand;
    std::vector<uint64_t> coff, pool_src(1, DEC_NO_COMMITTEE);
    std::vector<CopyPiece> pieces;
    pieces.reserve(n);
    be_set_slot(ctx, 0);
    LCV_TRY(ctx->dec_pin.grow(ctx, S.stage_bytes));
    LCV_TRY(ctx->dec_mem.grow(ctx, S.total));
    uint8_t* pin = ctx->dec_pin.p;
    uint8_t* d = ctx->dec_mem.p;
    {  // staging: the messages (host threads above 8 MB), the padding, the meta records
      uint64_t o = 0;
      for (uint64_t i = 0; i < n; ++i) {
        const uint32_t f = forks ? (uint32_t)forks[i] : (uint32_t)fork;
        const uint32_t len = (uint32_t)lengths[i];  // (<= LCV_DECODE_MAX_BYTES < 2^32)
        memcpy(pin + S.meta + DEC_META_BYTES * i, &o, 8);
        memcpy(pin + S.meta + DEC_META_BYTES * i + 8, &len, 4);
        memcpy(pin + S.meta + DEC_META_BYTES * i + 12, &f, 4);
        if (lengths[i]) pieces.push_back({pin + o, buf + offsets[i], (size_t)lengths[i]});
        o += (lengths[i] + 15) & ~(uint64_t)15;
      }
      memset(pin + o, 0, 16);
      copy_pieces(pieces, (size_t)msg_bytes);
    }
    be_reset_timings(ctx);
    LCV_TRY(be_h2d(ctx, d, pin, S.stage_bytes));
    DecArgs A = {d, d + S.meta, d + S.rec, ProdOut{}, (uint32_t)kind, (uint32_t)DEC_PLAN};
    if (kind == WIRE_UPDATE) {
      LCV_TRY(stage(ctx, ST_WIRE_DECODE, [&] { return be_launch_team(ctx, F_wire_dec{A}, (uint32_t)n); }));
      LCV_TRY(be_d2h(ctx, rec.data(), d + S.rec, n * DEC_REC_BYTES));
      LCV_TRY(be_sync(ctx));
      const uint32_t none = 0xffffffffu;
      rep.assign(n, none);
      coff.assign(n, 0);
      for (uint64_t i = 0; i < n; ++i) {
        uint32_t st, zero;
        memcpy(&st, rec.data() + DEC_REC_BYTES * i, 4);
        memcpy(&zero, rec.data() + DEC_REC_BYTES * i + 4, 4);
        if (st || zero) continue;
        uint64_t o;
        memcpy(&o, pin + S.meta + DEC_META_BYTES * i, 8);
        coff[i] = o + wire_committee_off((forks ? forks[i] : fork) == WIRE_ALTAIR);
        cand.push_back((uint32_t)i);
      }
      LCV_TRY(dec_resolve_pool(ctx, d, S, cand, rec.data(), coff, rep));
      std::vector<uint32_t> first;
      dedup_pool_rows(rep, nsc_index.data(), first);
      pool_src.clear();
      for (uint32_t f : first) pool_src.push_back(f == none ? DEC_NO_COMMITTEE : coff[f]);
    }
    const uint64_t npool = pool_src.size();
    // the batch: lcv_batch_upload's layout
    BatchCols c;
    batch_layout(c, n, npool, false, 0);
    NewBatch nb(ctx);
    LCV_TRY(batch_new(ctx, c, nb));
    uint8_t* m = nb.db->mem.p;
    LCV_TRY(be_h2d(ctx, m + c.off[COL_NSC_INDEX], nsc_index.data(), 4 * n));
    A.O = prod_out(nb.db->B);
    A.phase = DEC_ROWS;
    if (kind == WIRE_UPDATE) A.rec = nullptr;  // (the first pass left the records)
    LCV_TRY(stage(ctx, ST_WIRE_DECODE, [&] { return be_launch_team(ctx, F_wire_dec{A}, (uint32_t)n); }));
    if (kind == WIRE_UPDATE) {
      LCV_TRY(be_h2d(ctx, d + S.pool_src, pool_src.data(), 8 * npool));
      const ScGatherArgs G = {d, (const uint64_t*)(d + S.pool_src), m + c.off[COL_NSC_POOL]};
      LCV_TRY(stage(ctx, ST_DECODE_POOL, [&] { return be_launch_team(ctx, F_sc_gather{G}, (uint32_t)npool); }));
    } else {
      LCV_TRY(be_memset(ctx, m + c.off[COL_NSC_POOL], 0, K_SC));
      LCV_TRY(be_d2h(ctx, rec.data(), d + S.rec, n * DEC_REC_BYTES));
    }
    LCV_TRY(be_sync(ctx));
    be_collect_timings(ctx);
    for (uint64_t i = 0; i < n; ++i) status_out[i] = rec[DEC_REC_BYTES * i] ? 1 : 0;
    return nb.hand_out(out);
  });
}

// ------------------------------------------------------------------ the classes of a resident batch, and its fan-out
// lcv_batch_classify: dedup_classes' column for a batch whose rows never were on the host.  F_dedup_key gives every
// row a 64-bit key of its tuple, the host groups the keys alone (dedup_group under lcv_debug_dedup_hash_bits), and
// every row but a group's first is compared in full with its tentative representative on the device
// (F_dedup_confirm; dedup_confirm_groups splits the groups whose members differ).  Keys, pair lists and flags live
// in one Scratch of the call, sized for one piece of ctx->chunk rows or pairs; a longer batch takes several launches
int lcv_last_classify_timings(lcv_ctx* ctx, float ms_out[2]) {
  if (!ctx || !ms_out) return fail(ctx, LCV_EINVAL, "lcv_last_classify_timings: null argument");
  ms_out[0] = ctx->stage_ms[ST_CLASS_KEY];
  ms_out[1] = ctx->stage_ms[ST_CLASS_CONFIRM];
  return LCV_OK;
}

int lcv_debug_batch_classes(lcv_ctx* ctx, const lcv_dbatch* b, uint32_t* out) {
  if (!ctx || !b || !out) return fail(ctx, LCV_EINVAL, "lcv_debug_batch_classes: null argument");
  if (b->cls.size() != b->n || b->n == 0) return fail(ctx, LCV_EINVAL, "lcv_debug_batch_classes: the batch has no class column");
  memcpy(out, b->cls.data(), 4 * (size_t)b->n);
  return LCV_OK;
}

int lcv_batch_classify(lcv_ctx* ctx, lcv_dbatch* b, uint64_t* classes_out) {
  const char* who = "lcv_batch_classify";
  if (!ctx || !b || !classes_out) return fail(ctx, LCV_EINVAL, std::string(who) + ": null argument");
  *classes_out = 0;
  if (b->n == 0) return LCV_OK;
  return guarded(ctx, who, [&]() -> int {
    const size_t n = (size_t)b->n, piece = std::min(n, ctx->chunk);
    std::vector<uint64_t> key(n), sig_slot(n);
    std::vector<uint32_t> cls(n), store(b->B.store_index ? n : 0), pending, pairs;
    Layout l;
    const size_t o_key = l.take(8 * piece), o_pairs = l.take(8 * piece), o_differ = l.take(4 * piece);
    be_set_slot(ctx, 0);
    Scratch mem(ctx);
    LCV_TRY(mem.alloc(l.total()));
    uint64_t* key_dev = (uint64_t*)(mem.p + o_key);
    uint32_t* pairs_dev = (uint32_t*)(mem.p + o_pairs);
    uint32_t* differ_dev = (uint32_t*)(mem.p + o_differ);
    be_reset_timings(ctx);
    for (size_t base = 0; base < n; base += piece) {
      const uint32_t m = (uint32_t)std::min(piece, n - base);
      const F_dedup_key f = {chunk_view(b->B, base, m), key_dev};
      LCV_TRY(stage(ctx, ST_CLASS_KEY, [&] { return be_launch_team(ctx, f, m); }));
      LCV_TRY(be_d2h(ctx, key.data() + base, key_dev, 8 * (size_t)m));
    }
    // what the grouping at validate time reads of the rows (dedup_chunk, dedup_comm_rows), one copy per column
    LCV_TRY(be_d2h(ctx, sig_slot.data(), b->B.sig_slot, 8 * n));
    if (b->B.store_index) LCV_TRY(be_d2h(ctx, store.data(), b->B.store_index, 4 * n));
    LCV_TRY(be_sync(ctx));
    uint64_t classes = 0;
    dedup_group(
        (uint32_t)n, ctx->dedup_hash_bits, ctx->dd_table, [&](uint32_t i) { return key[i]; },
        [](uint32_t, uint32_t) { return true; }, [&](uint32_t i) { cls[i] = i; }, [&](uint32_t a, uint32_t i) { cls[i] = a; });
    for (size_t i = 0; i < n; ++i)
      if (cls[i] != i) pending.push_back((uint32_t)i);
    LCV_TRY(dedup_confirm_groups(cls, pending, [&](const std::vector<uint32_t>& pend, const std::vector<uint32_t>& rp,
                                                   std::vector<uint32_t>& differ) -> int {
      const size_t np = pend.size();
      pairs.resize(2 * np);
      for (size_t k = 0; k < np; ++k) {
        const uint32_t a = pend[k], c = rp[a];
        if (a >= n || c >= n) return fail(ctx, LCV_EINVAL, std::string(who) + ": pair " + std::to_string(k) + " names a row past the batch");
        pairs[2 * k] = a;
        pairs[2 * k + 1] = c;
      }
      for (size_t k0 = 0; k0 < np; k0 += piece) {
        const uint32_t m = (uint32_t)std::min(piece, np - k0);
        LCV_TRY(be_h2d(ctx, pairs_dev, pairs.data() + 2 * k0, 8 * (size_t)m));
        const F_dedup_confirm f = {b->B, pairs_dev, differ_dev};
        LCV_TRY(stage(ctx, ST_CLASS_CONFIRM, [&] { return be_launch_team(ctx, f, m); }));
        LCV_TRY(be_d2h(ctx, differ.data() + k0, differ_dev, 4 * (size_t)m));
      }
      return be_sync(ctx);
    }));
    be_collect_timings(ctx);
    for (size_t i = 0; i < n; ++i) classes += cls[i] == i;
    // (nothing fails from here on: a batch classed before keeps its columns when the call does not succeed)
    b->cls.swap(cls);
    b->h_sig_slot.swap(sig_slot);
    b->h_store.swap(store);
    *classes_out = classes;
    return LCV_OK;
  });
}

// lcv_batch_fan_out: row i of the new batch = row rows[i] of src (rows null: row i), gathered on the device
// (F_prod_pick, as lcv_batch_download's row list), the pool copied whole so that nsc_index stays valid, and the
// store_index column attached as lcv_batch_upload_stores does (bind_batch records its largest entry).  The classes of
// a classed source are inherited on the host: dedup_plan takes any labels
int lcv_batch_fan_out(lcv_ctx* ctx, lcv_dbatch* src, const uint32_t* rows, const uint32_t* store_index, uint64_t n,
                      lcv_dbatch** out) {
  const char* who = "lcv_batch_fan_out";
  if (out) *out = nullptr;
  if (!ctx || !src || !out) return fail(ctx, LCV_EINVAL, std::string(who) + ": null argument");
  if (!rows && !store_index) return fail(ctx, LCV_EINVAL, std::string(who) + ": rows and store_index are both null");
  if (n == 0 || n >= 0xffffffffull) return fail(ctx, LCV_EINVAL, std::string(who) + ": need 0 < n < 2^32 - 1");
  if (!rows && n != src->n)
    return fail(ctx, LCV_EINVAL, std::string(who) + ": without rows, n = " + std::to_string(n) + " must be the source's " +
                                     std::to_string(src->n) + " rows");
  if (rows) LCV_TRY(prod_check_index(ctx, who, "rows", rows, n, src->n));
  return guarded(ctx, who, [&]() -> int {
    // (a single-store batch classed at upload keeps no signature_slot column: a table batch made from it reads its own)
    const bool classed = !src->cls.empty(), slots = src->h_sig_slot.size() == src->n;
    std::vector<uint32_t> cls, h_store;
    std::vector<uint64_t> h_sig_slot;
    if (classed) {
      cls.resize(n);
      if (slots || store_index) h_sig_slot.resize(n);
      for (size_t i = 0; i < n; ++i) {
        const size_t s = rows ? rows[i] : i;
        cls[i] = src->cls[s];
        if (slots) h_sig_slot[i] = src->h_sig_slot[s];
      }
      if (store_index) h_store.assign(store_index, store_index + n);
    }
    BatchCols c;
    batch_layout(c, n, src->npool, store_index != nullptr, 0);
    c.src[COL_STORE_INDEX] = store_index;
    NewBatch nb(ctx);
    be_set_slot(ctx, 0);
    LCV_TRY(batch_new(ctx, c, nb));
    lcv_dbatch* db = nb.db;
    Scratch mem(ctx);  // (freed, waiting for the streams, ahead of an abandoned batch)
    if (rows) {
      LCV_TRY(mem.alloc(4 * n));
      LCV_TRY(be_h2d(ctx, mem.p, rows, 4 * n));
      LCV_TRY(be_launch_team(ctx, F_prod_pick{src->B, (const uint32_t*)mem.p, prod_out(db->B)}, (uint32_t)n));
    } else {
      for (const ColSpec& s : kBatchCols)
        if (col_per_row(s) && s.prod >= 0) LCV_TRY(be_d2d(ctx, slot_get(&db->B, s.dev), slot_get(&src->B, s.dev), s.width * n));
    }
    LCV_TRY(be_d2d(ctx, db->mem.p + c.off[COL_NSC_POOL], src->B.nsc_pool, c.bytes[COL_NSC_POOL]));
    LCV_TRY(be_h2d(ctx, db->mem.p + c.off[COL_STORE_INDEX], store_index, c.bytes[COL_STORE_INDEX]));
    if (classed && store_index && !slots) LCV_TRY(be_d2h(ctx, h_sig_slot.data(), db->B.sig_slot, 8 * n));
    LCV_TRY(be_sync(ctx));
    db->cls.swap(cls);
    db->h_sig_slot.swap(h_sig_slot);
    db->h_store.swap(h_store);
    return nb.hand_out(out);
  });
}

}  // extern "C"

// ------------------------------------------------------------------ the asynchronous relay (include/lcv.h; F_wire_relay,
// lcv_wire_dec.hpp).  What lcv_batch_decode -> lcv_batch_classify -> lcv_batch_fan_out -> lcv_validate_resident does in
// four synchronous calls on slot 0, enqueued on one slot without a wait: the slot's pinned region takes the messages (as
// lcv_batch_decode stages them), the meta records, the pair list and, where the modes ask for them, the grouping into BLS
// items (the plan_m path of dedup_chunk) and the grouping by store (the FoldReq path of validate_impl); one DMA moves it
// into the slot's device buffer, which holds behind it the status records and a table batch of npairs rows
// (batch_layout, one all-zero pool row, nsc_index all zero).  Both buffers are the HostSlot's, under stage_transit's rule
struct RelayLayout {
  size_t meta, rows, store, seg_store, seg_off, seg_row, seg_in, rep, urow, stage_bytes, rec, batch, total;
  BatchCols c;  // the table batch, at `batch` (its store_index column and its groupings are the staged ones)
};
static void relay_layout(RelayLayout& L, size_t msg_bytes, size_t nmsg, size_t np, size_t ng, size_t nd) {
  Layout l;
  l.take(msg_bytes);  // the messages, at offset 0
  L.meta = l.take(nmsg * DEC_META_BYTES);
  L.rows = l.take(4 * np);
  L.store = l.take(4 * np);
  L.seg_store = l.take(4 * ng);
  L.seg_off = l.take(ng ? 4 * (ng + 1) : 0);
  L.seg_row = l.take(ng ? 4 * np : 0);
  L.seg_in = l.take(sizeof(FoldState) * ng);
  L.rep = l.take(nd ? 4 * np : 0);
  L.urow = l.take(4 * nd);
  L.stage_bytes = l.total();  // what the one DMA moves
  L.rec = l.take(nmsg * DEC_REC_BYTES);
  L.batch = l.total();
  batch_layout(L.c, np, 1, false, 0);
  L.total = L.batch + L.c.total;
}

namespace lcv {  // lcv_wire.cpp: the host decoder's walk, storing the class tuple alone
void wire_dedup_tuples(const uint8_t* buf, const uint64_t* offsets, const uint64_t* lengths, uint64_t n, int kind, int fork,
                       const uint8_t* forks, uint8_t* beacon, uint8_t* bits, uint8_t* sig, uint64_t* slot);
}

// the pairs' grouping into BLS items, as the synchronous path makes it: dedup_classes over the messages' tuples (what
// lcv_batch_classify computes from the decoded rows), a pair's class its message's (lcv_batch_fan_out), the committee
// row from the pair's store and its message's signature_slot, dedup_plan (dedup_chunk).  Into the context's scratch
static void relay_plan(lcv_ctx* ctx, const lcv_relay_request* rq, DedupCols& dd) {
  const size_t nmsg = (size_t)rq->nmsg, np = (size_t)rq->npairs;
  ctx->rl_beacon.resize(nmsg * K_BEACON);
  ctx->rl_bits.resize(nmsg * K_BITS);
  ctx->rl_sig.resize(nmsg * K_SIG);
  ctx->rl_slot.resize(nmsg);
  ctx->rl_cls.resize(nmsg);
  ctx->rl_pslot.resize(np);
  ctx->dd_cls.resize(np);
  ctx->dd_comm.resize(np);
  ctx->dd_rep.resize(np);
  ctx->dd_urow.resize(np);
  wire_dedup_tuples(rq->buf, rq->offsets, rq->lengths, nmsg, rq->kind, rq->fork, rq->forks, ctx->rl_beacon.data(),
                    ctx->rl_bits.data(), ctx->rl_sig.data(), ctx->rl_slot.data());
  dedup_classes(ctx->rl_beacon.data(), ctx->rl_slot.data(), ctx->rl_bits.data(), ctx->rl_sig.data(), (uint32_t)nmsg,
                ctx->dedup_hash_bits, ctx->rl_cls.data(), ctx->dd_table);
  for (size_t i = 0; i < np; ++i) {
    ctx->dd_cls[i] = ctx->rl_cls[rq->rows[i]];
    ctx->rl_pslot[i] = ctx->rl_slot[rq->rows[i]];
  }
  dedup_comm_rows(ctx, rq->store_index, ctx->rl_pslot.data(), np, ctx->dd_comm.data());
  dd.m = dedup_plan(ctx->dd_cls.data(), ctx->dd_comm.data(), (uint32_t)np, ctx->dedup_hash_bits, ctx->dd_rep.data(),
                    ctx->dd_urow.data(), ctx->dd_table);
  dd.rep = ctx->dd_rep.data();
  dd.urow = ctx->dd_urow.data();
}

// the host copies of the staging step (host threads above 8 MB) into the slot's pinned region, laid out as L
static void relay_stage(uint8_t* pin, const RelayLayout& L, const lcv_relay_request* rq, const FoldSegs* segs,
                        const DedupCols& dd) {
  const size_t nmsg = (size_t)rq->nmsg, np = (size_t)rq->npairs;
  std::vector<CopyPiece> pieces;
  pieces.reserve(nmsg + 8);
  uint64_t o = 0;
  for (size_t j = 0; j < nmsg; ++j) {
    const uint32_t f = rq->forks ? (uint32_t)rq->forks[j] : (uint32_t)rq->fork;
    const uint32_t len = (uint32_t)rq->lengths[j];  // (<= LCV_RELAY_MAX_BYTES < 2^32)
    memcpy(pin + L.meta + DEC_META_BYTES * j, &o, 8);
    memcpy(pin + L.meta + DEC_META_BYTES * j + 8, &len, 4);
    memcpy(pin + L.meta + DEC_META_BYTES * j + 12, &f, 4);
    if (len) pieces.push_back({pin + o, rq->buf + rq->offsets[j], (size_t)len});
    o += ((uint64_t)len + 15) & ~(uint64_t)15;
  }
  memset(pin + o, 0, 16);
  auto col = [&](size_t at, const void* src, size_t bytes) {
    if (bytes) pieces.push_back({pin + at, (const uint8_t*)src, bytes});
  };
  col(L.rows, rq->rows, 4 * np);
  col(L.store, rq->store_index, 4 * np);
  if (segs) {
    col(L.seg_store, segs->store.data(), 4 * (size_t)segs->nseg);
    col(L.seg_off, segs->off.data(), 4 * ((size_t)segs->nseg + 1));
    col(L.seg_row, segs->row.data(), 4 * np);
    col(L.seg_in, segs->in.data(), sizeof(FoldState) * (size_t)segs->nseg);
  }
  if (dd.m) {
    col(L.rep, dd.rep, 4 * np);
    col(L.urow, dd.urow, 4 * (size_t)dd.m);
  }
  copy_pieces(pieces, L.stage_bytes);
}

extern "C" {

int lcv_relay_async(lcv_ctx* ctx, const lcv_relay_request* rq, int slot) {
  const std::string who = "lcv_relay_async";
  if (!ctx || !rq || !rq->buf || !rq->offsets || !rq->lengths || !rq->rows || !rq->store_index || !rq->genesis_validators_root)
    return fail(ctx, LCV_EINVAL, who + ": null argument");
  if (slot < 0 || slot >= LCV_SLOTS) return fail(ctx, LCV_EINVAL, who + ": slot must be 0..7");
  if (rq->kind != WIRE_FINALITY && rq->kind != WIRE_OPTIMISTIC)
    return fail(ctx, LCV_EINVAL, who + ": kind is 1 (finality) or 2 (optimistic); 0 (update) takes the synchronous path");
  if (!rq->forks && !wire_fork_ok(rq->fork)) return fail(ctx, LCV_EINVAL, who + ": fork is 0 (Deneb), 1 (Capella) or 2 (Altair)");
  const uint64_t nmsg = rq->nmsg, np = rq->npairs;
  if (nmsg == 0 || np == 0) return fail(ctx, LCV_EINVAL, who + ": need nmsg > 0 and npairs > 0");
  if (nmsg > LCV_DECODE_MAX_ROWS)
    return fail(ctx, LCV_EINVAL, who + ": nmsg = " + std::to_string(nmsg) + " above LCV_DECODE_MAX_ROWS");
  if (np > ctx->chunk)
    return fail(ctx, LCV_EINVAL, who + ": npairs = " + std::to_string(np) + " above one chunk of " + std::to_string(ctx->chunk) + " rows");
  uint64_t msg_bytes = 16;  // the zero padding behind the last message
  for (uint64_t j = 0; j < nmsg; ++j) {
    if (rq->lengths[j] > rq->buf_len || rq->offsets[j] > rq->buf_len - rq->lengths[j])
      return fail(ctx, LCV_EINVAL, who + ": message " + std::to_string(j) + ": offsets + lengths = " + std::to_string(rq->offsets[j]) +
                                       " + " + std::to_string(rq->lengths[j]) + " is past buf_len " + std::to_string(rq->buf_len));
    if (rq->lengths[j] <= LCV_RELAY_MAX_BYTES) msg_bytes += (rq->lengths[j] + 15) & ~(uint64_t)15;
    if (rq->lengths[j] > LCV_RELAY_MAX_BYTES || msg_bytes > LCV_RELAY_MAX_BYTES)
      return fail(ctx, LCV_EINVAL, who + ": staged bytes above LCV_RELAY_MAX_BYTES at message " + std::to_string(j));
  }
  LCV_TRY(prod_check_index(ctx, who.c_str(), "rows", rq->rows, np, nmsg));
  if (ctx->pipe_streams > 1)
    return fail(ctx, LCV_EINVAL, who + ": not with a multi-stream pipeline (lcv_set_pipeline streams > 1): sliced chains would need a grouping per slice");
  if (!ctx->table_set) return fail(ctx, LCV_ESTATE, who + ": lcv_set_store_table has not been called");
  LCV_TRY(store_index_check(ctx, who.c_str(), rq->store_index, np));
  return guarded(ctx, who.c_str(), [&]() -> int {
    // what the modes ask of the host, before anything is staged: the grouping by store (which checks the present
    // stores' states) and, with lcv_set_dedup on, the grouping into BLS items.  With the mode off nothing is parsed
    FoldReq req;
    const FoldSegs* segs = nullptr;
    if (rq->fold_in) {
      LCV_TRY(fold_segments(ctx, who.c_str(), rq->store_index, np, ctx->table_dev.nstore, rq->fold_in, ctx->segs));
      req.in = FoldState{};
      req.out = nullptr;  // the results wait in the slot's pinned area for lcv_slot_wait_relay
      req.segs = segs = &ctx->segs;
    }
    DedupCols dd = {nullptr, nullptr, 0};
    if (dedup_on(ctx)) relay_plan(ctx, rq, dd);
    const size_t ng = segs ? segs->nseg : 0;
    RelayLayout L;
    relay_layout(L, (size_t)msg_bytes, (size_t)nmsg, (size_t)np, ng, dd.m);
    const SlotResults r = {segs ? RES_RELAY_FOLD : RES_RELAY, (size_t)np, ng, (size_t)nmsg};
    HostSlot& h = ctx->slot[slot].host;
    LCV_TRY(stage_transit(ctx, slot, h, L.stage_bytes, L.total, results_offsets(r).total,
                          [&](uint8_t* pin) { relay_stage(pin, L, rq, segs, dd); }));
    uint8_t* d = h.dev.p;
    // the table batch: SyncCommittee() as its one pool row, every row's nsc_index 0
    bind_batch(&h.db, d + L.batch, L.c);
    h.db.B.store_index = (const uint32_t*)(d + L.store);
    for (size_t i = 0; i < np; ++i)
      if (rq->store_index[i] > h.db.max_store) h.db.max_store = rq->store_index[i];
    if (dd.m) {
      h.db.plan_rep = (const uint32_t*)(d + L.rep);
      h.db.plan_urow = (const uint32_t*)(d + L.urow);
      h.db.plan_m = dd.m;
    }
    if (segs) seg_bind(req, d, L.seg_store, L.seg_off, L.seg_row, L.seg_in);
    be_set_slot(ctx, slot);
    int rc = be_memset(ctx, d + L.batch + L.c.off[COL_NSC_POOL], 0, L.c.bytes[COL_NSC_POOL]);
    if (rc == LCV_OK) rc = be_memset(ctx, d + L.batch + L.c.off[COL_NSC_INDEX], 0, L.c.bytes[COL_NSC_INDEX]);
    if (rc == LCV_OK) {  // decode and fan-out in one launch: a team per pair, then a team per message for its status
      const DecArgs A = {d, d + L.meta, d + L.rec, prod_out(h.db.B), (uint32_t)rq->kind, (uint32_t)DEC_ROWS};
      const F_wire_relay f = {RelayDecArgs{A, (const uint32_t*)(d + L.rows), (uint32_t)np}};
      rc = be_relay_mark(ctx, 0);
      if (rc == LCV_OK) rc = be_launch_team(ctx, f, (uint32_t)(np + nmsg));
      if (rc == LCV_OK) rc = be_relay_mark(ctx, 1);
    }
    be_set_slot(ctx, 0);
    if (rc != LCV_OK) return rc;
    return slot_enqueue(ctx, slot, rq->current_slot, rq->genesis_validators_root, segs ? &req : nullptr, r, d + L.rec);
  });
}

int lcv_slot_wait_relay(lcv_ctx* ctx, int slot, uint8_t* status_out, uint8_t* verdict_out, uint8_t* reason_out,
                        lcv_fold_result* fold_out) {
  if (!ctx || slot < 0 || slot >= LCV_SLOTS) return fail(ctx, LCV_EINVAL, "lcv_slot_wait_relay: slot must be 0..7");
  const SlotResults& r = ctx->slot[slot].host.res;
  if (!r.relay()) return fail(ctx, LCV_ESTATE, "lcv_slot_wait_relay: the slot's last batch was not enqueued by lcv_relay_async");
  if (fold_out && r.kind != RES_RELAY_FOLD) return fail(ctx, LCV_ESTATE, "lcv_slot_wait_relay: the slot's relay was enqueued without fold_in");
  return slot_collect(ctx, slot, r.n, verdict_out, reason_out, fold_out, status_out);
}

int lcv_last_relay_timings(lcv_ctx* ctx, int slot, float ms_out[2]) {
  if (!ctx || !ms_out || slot < 0 || slot >= LCV_SLOTS)
    return fail(ctx, LCV_EINVAL, "lcv_last_relay_timings: null argument or slot not in 0..7");
  ms_out[1] = 0.f;
  return be_relay_ms(ctx, slot, &ms_out[0]);
}

}  // extern "C"
