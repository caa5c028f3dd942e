// lcv_backend.hpp — the execution backend the driver (lcv_driver.inc) runs on, declared once.
// Both backends define `struct Backend` and the LCV_HD qualifier of functor call operators, include this header,
// include the driver, and then define every function below: lcv_hip.hip over HIP streams, events and kernels
// on gfx950 (the product, liblcv.so), lcv_hostsim.cpp as plain host loops in program order (test-only; what
// orders nothing there — slots, events, forks — is a no-op stub).
#pragma once
#include <stddef.h>
#include <stdint.h>

struct lcv_ctx;

static int be_init(lcv_ctx* ctx, int device);
static void be_destroy(lcv_ctx* ctx);
// memory.  be_free waits for every stream first; be_host_alloc gives pinned memory, whose copies are DMA,
// asynchronous to the host.  Copies and be_memset are enqueued on the current stream
static int be_alloc(lcv_ctx* ctx, void** p, size_t bytes);
static void be_free(lcv_ctx* ctx, void* p);
static int be_host_alloc(lcv_ctx* ctx, void** p, size_t bytes);
static void be_host_free(lcv_ctx* ctx, void* p);
static int be_h2d(lcv_ctx* ctx, void* dst, const void* src, size_t bytes);
static int be_d2h(lcv_ctx* ctx, void* dst, const void* src, size_t bytes);
static int be_d2d(lcv_ctx* ctx, void* dst, const void* src, size_t bytes);
static int be_memset(lcv_ctx* ctx, void* p, int v, size_t bytes);
// launches on the current stream: one lane per item; one team per item; a SOP program on the batch engine (g
// items per one-wave block) or on the fan engine (one item per block)
template <class F> static int be_launch(lcv_ctx* ctx, const F& f, uint32_t n);
template <class F> static int be_launch_team(lcv_ctx* ctx, const F& f, uint32_t n);
template <class F> static int be_launch_sop(lcv_ctx* ctx, const F& f, uint32_t n, uint32_t g);
template <class F> static int be_launch_sop_fan(lcv_ctx* ctx, const F& f, uint32_t n);
// a SOP program on the batch engine over *n_dev <= n_max items: the count is device memory the stream's earlier
// kernels wrote, which the host does not wait for
template <class F> static int be_launch_sop_counted(lcv_ctx* ctx, const F& f, const uint32_t* n_dev, uint32_t n_max, uint32_t g);
// streams: work-space slot s owns a main stream (0) and a side stream (1), plus the forked streams of a sliced
// pipeline.  be_set_slot makes a slot's main stream current; be_use_stream picks stream k of the active slot
static void be_set_slot(lcv_ctx* ctx, int slot);
static void be_use_stream(lcv_ctx* ctx, int k);
// the active slot's ordering events (EV_*, lcv_common.hpp): recorded on stream k, waited for by stream k or
// (be_wait_event) by the host, which returns at once for an event never recorded
static int be_mark(lcv_ctx* ctx, int ev, int k);
static int be_wait(lcv_ctx* ctx, int k, int ev);
static int be_wait_event(lcv_ctx* ctx, int ev);
// stream k starts after the main stream's work so far / the main stream continues after stream k's
static int be_fork_to(lcv_ctx* ctx, int k);
static int be_join_from(lcv_ctx* ctx, int k);
static int be_sync(lcv_ctx* ctx);       // every stream of the context
static int be_sync_slot(lcv_ctx* ctx);  // the active slot's two streams
// stage marks (the driver's stage()): the time between a pair on one stream is added to ctx->stage_ms[stage] by
// be_collect_timings; nothing is recorded while ctx->marks_off
static void be_stage_begin(lcv_ctx* ctx, int stage);
static void be_stage_end(lcv_ctx* ctx, int stage);
static void be_reset_timings(lcv_ctx* ctx);
static void be_collect_timings(lcv_ctx* ctx);
static size_t be_event_pool_size(lcv_ctx* ctx);
// the asynchronous relay's own pair of marks per slot (lcv_last_relay_timings): recorded on the current stream whatever
// ctx->marks_off says, outside the event pool; be_relay_ms waits for the pair and gives the time between them (0 for
// a slot that never recorded one)
static int be_relay_mark(lcv_ctx* ctx, int end);
static int be_relay_ms(lcv_ctx* ctx, int slot, float* ms);
// the communicator (lcv_comm_*): collectives on the current stream, be_comm_wait bounded by ctx->comm_timeout_s
static int be_comm_unique_id(uint8_t* id);
static int be_comm_init(lcv_ctx* ctx, int nranks, int rank, const uint8_t* id);
static void be_comm_destroy(lcv_ctx* ctx);
static int be_comm_allgather(lcv_ctx* ctx, const uint8_t* send, uint8_t* recv, size_t per_rank);
static int be_comm_allreduce_max(lcv_ctx* ctx, double* inout);
static int be_comm_count(lcv_ctx* ctx, int* out);
static int be_comm_wait(lcv_ctx* ctx);
static int be_comm_shrink(lcv_ctx* ctx, const int* exclude, int nexclude, int* rank, int* nranks);
static void be_comm_abort(lcv_ctx* ctx);
