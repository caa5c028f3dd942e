/* lcv.h — C ABI of liblcv.so, the MI355X (gfx950) batched light-client verifier.
 *
 * Drop-in boundary for the hot path of Inspector-Butters/light-client-consensus-specs:
 *   validate_light_client_update(store, update, current_slot, genesis_validators_root)
 *       reference sync-protocol.md:386-465           -> lcv_set_store + lcv_validate_updates
 *   bls.FastAggregateVerify(pubkeys, message, signature)
 *       reference call site sync-protocol.md:464      -> lcv_fast_aggregate_verify(_batch)
 *   is_valid_merkle_branch(leaf, branch, depth, index, root)
 *       reference call sites sync-protocol.md:234,356,428,443 -> lcv_merkle_branch_batch
 *   hash_tree_root(SyncCommittee)
 *       reference call site sync-protocol.md:444      -> lcv_htr_sync_committee_batch
 *
 * Conventions: plain pointers and sizes, caller owns every host buffer, the library copies in and
 * out.  Every function returns 0 (LCV_OK) or a negative lcv_status; lcv_last_error() explains.
 * No C++ exception crosses the ABI.  One lcv_ctx per device, not shared between threads.
 * Byte layouts of the packed update batch (structure of arrays, one row per update) are given
 * next to lcv_update_batch and in DESIGN.md.
 */
#ifndef LCV_H
#define LCV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCV_SYNC_COMMITTEE_SIZE 512
#define LCV_PUBKEY_BYTES 48
#define LCV_SIGNATURE_BYTES 96
#define LCV_SYNC_COMMITTEE_BYTES 24624 /* SSZ SyncCommittee: 512 x 48 B pubkeys + 48 B aggregate */
#define LCV_BEACON_HEADER_BYTES 112    /* SSZ BeaconBlockHeader */
#define LCV_EXEC_RECORD_BYTES 832      /* packed ExecutionPayloadHeader, see below */
#define LCV_EXEC_BRANCH_BYTES 128      /* ExecutionBranch 4 x 32 */
#define LCV_NSC_BRANCH_BYTES 160       /* NextSyncCommitteeBranch 5 x 32 */
#define LCV_FINALITY_BRANCH_BYTES 192  /* FinalityBranch 6 x 32 */
#define LCV_SYNC_BITS_BYTES 64         /* SSZ Bitvector[512] */

enum lcv_status { LCV_OK = 0, LCV_EINVAL = -1, LCV_EDEVICE = -2, LCV_ENOMEM = -3, LCV_ESTATE = -4 };

/* reason codes: k = the k-th assert of validate_light_client_update in source order */
enum lcv_reason {
  LCV_VALID = 0,
  LCV_R_PARTICIPANTS = 1,            /* :392 */
  LCV_R_ATTESTED_HEADER = 2,         /* :395 */
  LCV_R_SLOT_ORDER = 3,              /* :398 */
  LCV_R_SIG_PERIOD_NEXT_KNOWN = 4,   /* :402 */
  LCV_R_SIG_PERIOD_NEXT_UNKNOWN = 5, /* :404 */
  LCV_R_NOT_RELEVANT = 6,            /* :411-414 */
  LCV_R_FINALIZED_NOT_EMPTY = 7,     /* :420 */
  LCV_R_FINALIZED_GENESIS = 8,       /* :423 */
  LCV_R_FINALIZED_HEADER = 9,        /* :426 */
  LCV_R_FINALITY_BRANCH = 10,        /* :428-434 */
  LCV_R_NSC_NOT_EMPTY = 11,          /* :439 */
  LCV_R_NSC_MISMATCH = 12,           /* :442 */
  LCV_R_NSC_BRANCH = 13,             /* :443-449 */
  LCV_R_SIGNATURE = 14               /* :464 */
};

typedef struct lcv_ctx lcv_ctx;
typedef struct lcv_dbatch lcv_dbatch;

/* Packed ExecutionPayloadHeader record (832 B): 17 SSZ leaf chunks of 32 B in field order
 * (parent_hash, fee_recipient (20 B + 12 zero), state_root, receipts_root, [leaf 4 unused: zero],
 * prev_randao, block_number, gas_limit, gas_used, timestamp (uint64 LE + 24 zero),
 * extra_data (zero padded), base_fee_per_gas (uint256 LE), block_hash, transactions_root,
 * withdrawals_root, blob_gas_used, excess_blob_gas), then logs_bloom (256 B) at offset 544,
 * extra_data length (uint32 LE) at 800, 28 zero bytes.  All-zero == ExecutionPayloadHeader(). */
typedef struct lcv_header_cols {
  const uint8_t* beacon;      /* n x 112 */
  const uint8_t* execution;   /* n x 832 */
  const uint8_t* exec_branch; /* n x 128 */
} lcv_header_cols;

typedef struct lcv_update_batch {
  lcv_header_cols attested;
  lcv_header_cols finalized;
  const uint8_t* nsc_pool;        /* npool x 24624: distinct next_sync_committee values */
  const uint32_t* nsc_index;      /* n: pool row holding update i's next_sync_committee */
  const uint8_t* nsc_branch;      /* n x 160 */
  const uint8_t* finality_branch; /* n x 192 */
  const uint8_t* sync_bits;       /* n x 64 */
  const uint8_t* sync_signature;  /* n x 96 */
  const uint64_t* signature_slot; /* n */
  uint64_t n;
  uint64_t npool;
} lcv_update_batch;

/* ---- context */
int lcv_device_count(int* out);
int lcv_init(int device, lcv_ctx** out);
void lcv_destroy(lcv_ctx* ctx);
const char* lcv_last_error(const lcv_ctx* ctx);

/* ---- network configuration, runtime (mainnet by default): the values sync-protocol.md reads from
 * the preset / config — SLOTS_PER_EPOCH and EPOCHS_PER_SYNC_COMMITTEE_PERIOD (periods, UPDATE_TIMEOUT),
 * fork_epochs4 = ALTAIR, BELLATRIX, CAPELLA, DENEB _FORK_EPOCH (is_valid_light_client_header :220-240,
 * get_lc_execution_root :186-214, compute_fork_version :461), fork_versions20 = GENESIS, ALTAIR,
 * BELLATRIX, CAPELLA, DENEB _FORK_VERSION (5 x 4 B), domain_sync_committee4 = DOMAIN_SYNC_COMMITTEE
 * (:462).  Fork epochs non-decreasing.  Applies to every later validate / bootstrap call on ctx.
 * SYNC_COMMITTEE_SIZE is the mainnet preset's 512 (the packed layouts above). */
int lcv_set_config(lcv_ctx* ctx, uint64_t slots_per_epoch, uint64_t epochs_per_sync_committee_period,
                   const uint64_t* fork_epochs4, const uint8_t* fork_versions20, const uint8_t* domain_sync_committee4);

/* ---- validate_light_client_update (sync-protocol.md:386-465) against one store snapshot.
 * The store's two committees (SSZ SyncCommittee bytes; an all-zero next committee means
 * "not known", sync-protocol.md:316-317) are decoded and KeyValidated once, device resident.
 * key_status_out (optional, 1024 B): 0 valid key, 2 invalid. */
int lcv_set_store(lcv_ctx* ctx, uint64_t finalized_slot, const uint8_t* current_sync_committee,
                  const uint8_t* next_sync_committee, uint8_t* key_status_out);
/* host batch in, verdict (1 = valid) and reason code (lcv_reason) out, one byte per update */
int lcv_validate_updates(lcv_ctx* ctx, const lcv_update_batch* batch, uint64_t current_slot,
                         const uint8_t* genesis_validators_root, uint8_t* verdict_out, uint8_t* reason_out);
/* ---- a store per update: the store table.  lcv_set_store holds ONE snapshot, and every row of a batch is
 * validated against it.  Two uses of the reference do not fit that: catching up over sync-committee periods
 * (light-client.md step 4.2, p2p-interface.md LightClientUpdatesByRange: one update per period, each meeting the
 * store the previous one left, whose committees have rotated), and serving light clients whose stores differ.
 * The table form: `committees` are the distinct SSZ SyncCommittee values (any order, duplicates allowed), a store
 * row s is (finalized_slot[s], current[s], next[s]) with the committees given as rows of that table, and update i
 * is validated against store row store_index[i].  next[s] = LCV_STORE_NEXT_UNKNOWN, or a committee row whose
 * 24624 bytes are all zero, means "not known" (sync-protocol.md:316-317), as lcv_set_store's all-zero next does.
 * lcv_set_store_table copies the committees to the device, decodes and KeyValidates all ncomm x 512 keys once
 * (key_status_out, optional, ncomm x 512: 0 valid key, 2 invalid; kernel time in lcv_last_timings' "setup"
 * stage) and keeps the store columns device resident.  It is independent of lcv_set_store: neither call touches
 * what the other set.  Both calls check every index on the host before any kernel is launched — current[s] <
 * ncomm, next[s] < ncomm or the sentinel, ncomm <= LCV_STORE_TABLE_MAX_COMMITTEES, store_index[i] < nstore — and
 * return LCV_EINVAL naming the first offending index; lcv_validate_updates_stores before a table is set returns
 * LCV_ESTATE.
 * lcv_validate_updates_stores is synchronous, host buffers in and out, like lcv_validate_updates: batches above
 * the chunk size are cut the same way, batches of at most lcv_set_latency_mode's rows run on the fan engine, and
 * lcv_set_pipeline applies.  Verdicts and reasons are those of lcv_set_store(store row) +
 * lcv_validate_updates(update), row by row.
 * Every other shape takes table batches too.  lcv_batch_upload_stores makes a resident batch that carries its
 * store_index column; no table needs to be set at that time, and the batch's largest index is recorded on the
 * host.  lcv_validate_resident, _resident_dev, _resident_async and lcv_validate_sharded (with lcv_slot_wait and
 * lcv_slot_allgather behind them) validate such a batch against the store table that is set when they are
 * called, and a batch from lcv_batch_upload against lcv_set_store, as ever.  Before any launch they check on the
 * host, in O(1): no table set -> LCV_ESTATE; recorded largest index >= the table's nstore -> LCV_EINVAL, naming
 * both numbers — a resident batch may outlive the table it was made for.  lcv_validate_stores_async is
 * lcv_validate_async with the store_index column staged: every index is checked on the host before the DMA
 * (LCV_EINVAL naming the first offending row, as lcv_validate_updates_stores), and lcv_slot_wait hands the results
 * out.  A single-store batch and a table batch may be in flight on different slots at once.
 * Ordering: lcv_set_store_table first waits for every work-space slot (all 8), then rewrites the table.  A
 * batch enqueued before the call finishes under the table it was enqueued under (its results stay in its slot
 * for lcv_slot_wait); work enqueued after the call sees the new table.  lcv_set_store does not wait: call it
 * with no single-store batch in flight. */
#define LCV_STORE_NEXT_UNKNOWN 0xFFFFFFFFu
#define LCV_STORE_TABLE_MAX_COMMITTEES 4096
typedef struct lcv_store_table {
  const uint8_t* committees;      /* ncomm x 24624 SSZ SyncCommittee, any order, duplicates allowed */
  uint64_t ncomm;
  const uint64_t* finalized_slot; /* nstore: store.finalized_header.beacon.slot */
  const uint32_t* current;        /* nstore: committee row of store.current_sync_committee */
  const uint32_t* next;           /* nstore: committee row of store.next_sync_committee, or LCV_STORE_NEXT_UNKNOWN */
  uint64_t nstore;
} lcv_store_table;
int lcv_set_store_table(lcv_ctx* ctx, const lcv_store_table* table, uint8_t* key_status_out);
int lcv_validate_updates_stores(lcv_ctx* ctx, const lcv_update_batch* batch, const uint32_t* store_index,
                                uint64_t current_slot, const uint8_t* genesis_validators_root,
                                uint8_t* verdict_out, uint8_t* reason_out);
/* ---- process_light_client_update after validation (sync-protocol.md:514-553), folded over a batch on the device
 * for ONE store: best update, max participants, optimistic header, and the first row that applies.  No per-row
 * host work remains; the host applies the one applying row with its own apply_light_client_update.
 *
 * The rank record (LCV_RANK_BYTES = 32, little-endian), one per update, written by lcv_rank_updates and, inside
 * the _fold calls, next to the pre-checks:
 *   u32 key0 : bit 23     super  = 3 n >= 2 * 512              (n = number of set sync_committee_bits)
 *              bits 22-13 super ? 0 : n
 *              bit 12     nsc_branch != 0  &&  period(attested slot) == period(signature_slot)
 *              bit 11     fin    = finality_branch != 0
 *              bit 10     fin && period(finalized slot) == period(attested slot)
 *              bits 9-0   n
 *   u32 flags: bit 0      is_sync_committee_update (nsc_branch != 0, without the period test)
 *   u64 attested_slot, u64 signature_slot, u64 finalized_slot
 * is_better_update(a, b) (sync-protocol.md:260-311, level by level) holds iff
 *   (key0_a, -attested_a, -signature_a) > (key0_b, -attested_b, -signature_b)   lexicographically;
 * equal triples mean "not better", so "the first best wins" is the first arg-max of the triple.
 * lcv_rank_updates reads six columns of the batch only — sync_bits, nsc_branch, finality_branch, attested.beacon
 * and finalized.beacon (their first 8 bytes: the slot), signature_slot — and uploads only those; every other
 * pointer of the batch is ignored and may be NULL.  Any n > 0, no store needed; the periods are lcv_set_config's.
 *
 * The fold.  Input: the batch's rank records and verdicts, the store values validation already holds
 * (lcv_set_store's finalized slot and whether its next committee is known) and the 48-byte fold state: the
 * store's optimistic slot, its two max_active_participants, and the rank of its best_valid_update if it has one.
 * Let t be the first row with verdict 1, `super`, and (finalized_slot > store finalized slot, or (next committee
 * not known and flags bit 0 and key0 bits 11 and 10)): the row process_light_client_update applies (:545-553).
 * Rows after t are not consumed: rows_consumed = t + 1, or n without such a row.  Over the valid rows <= t:
 *   - current_max_active_participants becomes the running max of n, seeded with the state's (:528-531);
 *   - the optimistic candidate is the first row attaining the largest attested_slot among the rows with
 *     n_i > max(previous_max, running_max_i) / 2 (integer division; running_max_i includes row i) and
 *     attested_slot > the state's optimistic_slot (:534-539): optimistic_row, next.optimistic_slot;
 *   - the best is the first arg-max of the rank, the state's own best winning ties (:521-525): best_row (-1 when
 *     the state's best stays, or there is none), next.has_best / best_*.
 * When a row applies, best_row is -1 and next.has_best is 0 (store.best_valid_update = None, :553), apply_row = t.
 * next's maxima and optimistic slot are the values BEFORE apply_light_client_update(row t), which the host runs.
 * accepted_count is the number of rows <= t (or of all rows) with verdict 1.  Results are bit-identical to looping
 * the reference over rows 0 .. rows_consumed - 1.
 *
 * lcv_validate_fold is lcv_validate_updates + the fold of that batch, chained behind the verdicts on the batch's
 * own stream (batch engine, fan engine and lcv_set_pipeline alike); the result travels back with the verdicts.
 * n <= LCV_FOLD_MAX_ROWS, else LCV_EINVAL: the caller cuts larger batches and carries `next` forward while
 * apply_row is -1.  lcv_validate_async_fold is lcv_validate_async with the fold; lcv_slot_wait_fold is
 * lcv_slot_wait plus the result, and returns LCV_ESTATE for a slot whose batch was not enqueued with a fold.
 * lcv_debug_fold (test hook) runs the fold alone on caller-supplied records and verdicts, no validation.
 * A batch with a store_index is refused by these entries (LCV_EINVAL): its fold is the segmented fold below.
 *
 * The segmented fold: one call validates a store-table batch and folds it per store.  A segment is the subsequence
 * of the batch's rows that share one store_index value s, in batch order; the rows of different stores may
 * interleave in any way, and segments are independent (a row that applies in one store consumes nothing in
 * another).  For every store s with at least one row, out[s] is exactly the fold above of that subsequence, run
 * against store row s of the table (its finalized slot; next committee known iff next[s] is a committee row that
 * is not all zero) from the state in[s], except that apply_row, best_row and optimistic_row are BATCH row numbers
 * (-1: none); rows_consumed and accepted_count count rows of the segment.  Row i of store s is consumed iff
 * out[s].apply_row < 0 || i <= out[s].apply_row.  `in` and `out` have one entry per store row of the table; only
 * the entries of stores that have a row in the batch are read, and only those are written: out[s] of a store with
 * no row is left untouched.  The host groups the rows by store in the pass that checks the indices (O(n log n),
 * independent of nstore); the grouping and the present stores' states travel with the batch's columns in its one
 * host-to-device copy, one 64-lane team per store present folds behind the verdicts (lcv_last_timings: the
 * store_fold stage), and 128 bytes per store present travel back with the verdicts.  A slot's result buffer is
 * allocated by its first segmented fold.
 * lcv_validate_stores_fold is lcv_validate_updates_stores + that fold (n <= LCV_FOLD_MAX_ROWS and one chunk, else
 * LCV_EINVAL; LCV_ESTATE without a table; LCV_EINVAL naming the row of a store_index >= nstore, or the store of a
 * present in[s] whose maxima exceed 512 — all before any launch).  lcv_validate_stores_async_fold is
 * lcv_validate_stores_async with it; lcv_slot_wait_stores_fold collects it and returns LCV_ESTATE for a slot not
 * enqueued by lcv_validate_stores_async_fold, as lcv_slot_wait_fold does for a slot that was; lcv_slot_wait hands
 * out such a slot's verdicts and reasons as for any staged batch.  lcv_debug_fold_stores (test hook) runs the
 * kernel alone on caller-supplied records, verdicts, store rows and per-store values: no validation, no table.
 * Out of scope, refused or absent: a fold of a resident table batch (lcv_batch_upload_stores), a sharded fold,
 * lcv.serving.validate_stream does not fold, and lcv.store.sync_light_client_updates does not (its rows are one
 * logical store at successive times, so their fold states chain). */
#define LCV_RANK_BYTES 32
#define LCV_FOLD_MAX_ROWS 65536
typedef struct lcv_fold_state {
  uint64_t optimistic_slot;                  /* store.optimistic_header.beacon.slot */
  uint64_t previous_max_active_participants;
  uint64_t current_max_active_participants;
  uint32_t has_best;                         /* store.best_valid_update is not None; then its rank: */
  uint32_t best_key0;
  uint64_t best_attested_slot;
  uint64_t best_signature_slot;
} lcv_fold_state;
typedef struct lcv_fold_result {
  lcv_fold_state next;
  uint64_t rows_consumed;
  int64_t apply_row, best_row, optimistic_row; /* -1: none */
  uint64_t accepted_count;
} lcv_fold_result;
int lcv_rank_updates(lcv_ctx* ctx, const lcv_update_batch* batch, uint8_t* rank_out /* n x 32 */);
int lcv_validate_fold(lcv_ctx* ctx, const lcv_update_batch* batch, uint64_t current_slot,
                      const uint8_t* genesis_validators_root, const lcv_fold_state* in, uint8_t* verdict_out,
                      uint8_t* reason_out, lcv_fold_result* out);
int lcv_validate_async_fold(lcv_ctx* ctx, const lcv_update_batch* batch, uint64_t current_slot,
                            const uint8_t* genesis_validators_root, const lcv_fold_state* in, int slot);
int lcv_slot_wait_fold(lcv_ctx* ctx, int slot, uint64_t n, uint8_t* verdict_out, uint8_t* reason_out,
                       lcv_fold_result* out);
int lcv_debug_fold(lcv_ctx* ctx, const uint8_t* rank /* n x 32 */, const uint8_t* verdict, uint64_t n,
                   uint64_t store_finalized_slot, int next_known, const lcv_fold_state* in, lcv_fold_result* out);
int lcv_validate_stores_fold(lcv_ctx* ctx, const lcv_update_batch* batch, const uint32_t* store_index,
                             uint64_t current_slot, const uint8_t* genesis_validators_root,
                             const lcv_fold_state* in /* nstore, indexed by store row */, uint8_t* verdict_out,
                             uint8_t* reason_out, lcv_fold_result* out /* nstore, entries of present stores written */);
int lcv_validate_stores_async_fold(lcv_ctx* ctx, const lcv_update_batch* batch, const uint32_t* store_index,
                                   uint64_t current_slot, const uint8_t* genesis_validators_root,
                                   const lcv_fold_state* in, int slot);
int lcv_slot_wait_stores_fold(lcv_ctx* ctx, int slot, uint64_t n, uint8_t* verdict_out, uint8_t* reason_out,
                              lcv_fold_result* out /* nstore */);
int lcv_debug_fold_stores(lcv_ctx* ctx, const uint8_t* rank /* n x 32 */, const uint8_t* verdict,
                          const uint32_t* store_index, uint64_t n, const uint64_t* store_finalized_slot /* nstore */,
                          const uint8_t* next_known /* nstore */, uint64_t nstore, const lcv_fold_state* in,
                          lcv_fold_result* out);
/* device-resident batches: upload once, validate many times (timed region excludes the upload) */
int lcv_batch_upload(lcv_ctx* ctx, const lcv_update_batch* batch, lcv_dbatch** out);
/* the same with the batch's store_index column (n entries): a table batch, see the store table above */
int lcv_batch_upload_stores(lcv_ctx* ctx, const lcv_update_batch* batch, const uint32_t* store_index, lcv_dbatch** out);
void lcv_batch_free(lcv_ctx* ctx, lcv_dbatch* b);
/* a resident batch's rows and pool rows (what lcv_batch_download's arrays hold): a batch the device made, as
 * lcv_batch_decode's, has a pool size only the batch knows */
int lcv_batch_shape(lcv_ctx* ctx, const lcv_dbatch* b, uint64_t* n_out, uint64_t* npool_out);
int lcv_validate_resident(lcv_ctx* ctx, lcv_dbatch* b, uint64_t current_slot, const uint8_t* genesis_validators_root,
                          uint8_t* verdict_out, uint8_t* reason_out);
/* same, verdicts written to a DEVICE buffer of n bytes (for an RCCL all-gather); no host copy */
int lcv_validate_resident_dev(lcv_ctx* ctx, lcv_dbatch* b, uint64_t current_slot,
                              const uint8_t* genesis_validators_root, uint8_t* verdict_dev);
/* Several batches in flight (multi-buffered serving loop; no reference counterpart: the reference
 * validates one update per call, sync-protocol.md:386).  lcv_validate_resident_async enqueues the whole
 * pipeline for b (at most 65536 updates) on the two HIP streams of work-space slot `slot` (0..7) and
 * returns without waiting; lcv_slot_wait waits for that slot and copies the first n verdicts / reason
 * codes out (either pointer may be NULL).  A slot's next batch starts on the device after its previous
 * one; alternate the slots and wait for a slot before reading or reusing it.  Synchronous calls use
 * slot 0 (and, for batches of several 64k chunks, every slot): wait for pending slots before them. */
int lcv_validate_resident_async(lcv_ctx* ctx, lcv_dbatch* b, uint64_t current_slot,
                                const uint8_t* genesis_validators_root, int slot);
int lcv_slot_wait(lcv_ctx* ctx, int slot, uint64_t n, uint8_t* verdict_out, uint8_t* reason_out);
/* Host-input serving entry (the per-batch form of lcv_validate_updates; callers sync-protocol.md:512 per
 * update and the gossip / Req/Resp ingress p2p-interface.md:69,99 per batch): the batch (at most 65536
 * updates) is copied into slot `slot`'s pinned staging buffer, uploaded by one DMA on the slot's stream
 * (overlapping the other slots' kernels), validated, and its verdicts / reasons copied back to pinned
 * memory — all enqueued without waiting; lcv_slot_wait(slot) waits and copies them out.  The caller's
 * buffers may be reused as soon as the call returns. */
int lcv_validate_async(lcv_ctx* ctx, const lcv_update_batch* batch, uint64_t current_slot,
                       const uint8_t* genesis_validators_root, int slot);
/* the same against the store table: update i against store row store_index[i] */
int lcv_validate_stores_async(lcv_ctx* ctx, const lcv_update_batch* batch, const uint32_t* store_index,
                              uint64_t current_slot, const uint8_t* genesis_validators_root, int slot);
/* multi-GPU form of lcv_slot_wait: after slot `slot`'s batch (n <= per_rank rows), all-gather every rank's
 * verdict bytes over RCCL (rank-major, each slice zero padded to per_rank) into verdict_all_out
 * (nranks * per_rank bytes) and wait.  Collective: every rank calls it in the same order. */
int lcv_slot_allgather(lcv_ctx* ctx, int slot, uint64_t n, uint64_t per_rank, uint8_t* verdict_all_out);
/* Execution shape of lcv_validate_*: each 64k-update chunk is cut into `chunks` slices whose whole
 * stage chains run on min(streams, 4) HIP streams, so different slices' kernels overlap.  streams = 1
 * (default) runs the stages one after another over the whole chunk (per-stage timings available);
 * verdicts are identical either way.  Performance knob only, no reference counterpart. */
int lcv_set_pipeline(lcv_ctx* ctx, int streams, int chunks);
/* Latency mode for small batches (the reference's per-update usage: validate_light_client_update and
 * bls.FastAggregateVerify once per update, sync-protocol.md:512, :464): calls whose batch (or chunk) has
 * at most max_rows rows run
 *   - the SOP programs (hash_to_G2 tail, final exponentiation) on the fan engine — an op's K products on
 *     K lanes and its reduction and tail on a 16-lane row, one update per block — instead of one op per lane,
 *   - both Miller line walks and the accumulation as ONE fan-engine program (lines through LDS), and
 *   - the SSWU maps and the signature decoding on their one-item-per-wave twins (each square-root
 *     product spread over the 64 lanes of a wave).
 * Results are identical to the batch engine's (bit for bit).  Default 64: one update 2.8 ms through
 * lcv_validate_updates on the MI355X (6.0 ms on the batch engine); 0 = the batch engine
 * always.  Performance knob only. */
int lcv_set_latency_mode(lcv_ctx* ctx, uint64_t max_rows);
/* test hook: which engines ran since the last reset (reset != 0 clears after reading).  out8[0] fan-engine
 * SOP launches, [1] batch-engine SOP launches, [2] one-item-per-wave twin launches (SSWU / signature),
 * [3] one-lane-per-item SSWU / signature launches, [4..7] items per wave of the last batch-engine launch of
 * the line walk, Miller accumulation, final exponentiation, hash_to_G2 tail (0 = not launched) */
int lcv_debug_engine_log(lcv_ctx* ctx, uint64_t* out8, int reset);
/* ---- Deduplicated signatures: each distinct sync-committee signature of a chunk checked once.  A light-client
 * server relays the same gossip messages and by-range responses to many clients: a finality update sent to 10^4
 * clients is 10^4 rows with the same attested header, signature_slot, sync_committee_bits and signature, which
 * differ only in store_index — and almost all of their stores hold the same current committee.  lcv_set_dedup(on)
 * (default 0: every call launches exactly what it launches without this mode) makes the BLS half of validation —
 * signing root, signature decode and subgroup check, hash_to_G2, masked aggregation, both Miller walks, final
 * exponentiation — run once per distinct BLS ITEM of a chunk; every row takes its verdict from its item.
 * The BLS item of a row is the tuple (attested beacon header 112 B, signature_slot, sync_bits 64 B,
 * sync_signature 96 B, the committee row the signature is checked against).  Those stages read nothing else of a
 * row (configuration and genesis_validators_root are per call), so rows with equal tuples have bytewise-equal
 * inputs to every BLS stage and bit-identical results.  Rows are merged only on a full compare of the tuple bytes,
 * never on a hash alone; rows whose tuples differ are never merged; and being conservative is allowed: two rows of
 * the committee table with equal content count as different committees.  The pre-checks (slots, periods,
 * relevance, Merkle branches, committee equality) depend on the row's own store and run for every row, as do the
 * rank records of the fold calls; verdict and reason bytes are per row, in the same places, so the folds,
 * lcv_slot_wait*, lcv_slot_allgather and lcv_validate_sharded work unchanged, and results equal the mode-off
 * results byte for byte.
 * Host side, O(n): when host columns enter the library with the mode on — lcv_validate_updates, _updates_stores,
 * _async, _stores_async, the four _fold entries, lcv_batch_upload and lcv_batch_upload_stores — every row gets a
 * store-independent class (equal attested beacon, signature_slot, bits, signature: a hash table, full compare on a
 * hash match).  At validate time, per chunk, the class is refined by the committee row the signature is checked
 * against — nothing to add for lcv_set_store (the choice depends on signature_slot only, which is in the class); for
 * a table batch, the row item_pre_table chooses under the store table of that call (a next committee that is not
 * known is a value like any other) — which gives rep[row] = item, urow[item] = its first row (ascending: items are
 * numbered by first appearance) and m, the number of items.  A staged host batch carries the two columns in its
 * one host-to-device copy; a resident batch keeps its class column on the host (4 B per row; a table batch also its
 * store_index and signature_slot columns, 12 B per row, which the committee choice reads) and each validation
 * sends the chunk's two columns in one small copy each.  A batch uploaded while the mode was off has no class column
 * and is validated without deduplication.  m is known before anything is launched, and launch sizes, items per
 * wave and the engine choice (lcv_set_latency_mode) go by m: 10^4 rows holding <= 64 distinct items run on the
 * fan engine.
 * Device side: after the pre-checks a gather kernel writes the items' four columns and committee ids into compact
 * scratch of the slot (284 B per item and 8 B per row, allocated by the slot's first deduplicated call), the BLS
 * stages run unchanged over those m items, and the verdict kernel reads the BLS flags of row i at rep[i].
 * lcv_set_dedup(on) together with a multi-stream pipeline (lcv_set_pipeline streams > 1) is refused with
 * LCV_EINVAL, by whichever call comes second: sliced chains would need a grouping per slice.
 * lcv_last_dedup reports the rows and items of the last batch enqueued on work-space slot `slot` (synchronous
 * calls: slot 0, summed over the batch's chunks); items == rows with the mode off or for a batch without a class
 * column (and in the CPU-baseline build, whose direct path runs every row).
 * lcv_debug_dedup_hash_bits is a test hook: the host hash is truncated to `bits` bits (default 64; 0 makes every
 * row collide, so that only the full compare separates classes).
 * Resident batches made on the device (lcv_create_updates_resident, lcv_batch_decode, lcv_batch_fan_out of an
 * unclassed batch) have no host bytes to class: they run without deduplication until lcv_batch_classify (below) has
 * classed them where they lie.
 * Out of scope: merging across chunks or across batches in flight; lcv_fast_aggregate_verify_batch;
 * merging committee-table rows of equal content; skipping the BLS work of items all of whose rows failed a
 * pre-check. */
int lcv_set_dedup(lcv_ctx* ctx, int on);
int lcv_last_dedup(lcv_ctx* ctx, int slot, uint64_t* rows, uint64_t* items);
int lcv_debug_dedup_hash_bits(lcv_ctx* ctx, int bits);
/* ---- Classes of a resident batch, made on the device; fanning a resident batch out to stores.  A relay keeps its
 * rows on the device: bytes -> lcv_batch_decode -> lcv_batch_classify -> lcv_batch_fan_out(rows, store_index) ->
 * lcv_validate_resident* under lcv_set_dedup -> lcv_batch_encode(rows = accepted); the host never holds a row and each
 * distinct signature is checked once.
 * lcv_batch_classify gives any resident batch (uploaded, decoded, created, fanned out), whatever lcv_set_dedup says, the
 * class column a batch uploaded with the mode on has: cls[i] = the first row whose (attested beacon header,
 * signature_slot, sync_bits, sync_signature) equal row i's, bytewise.  A kernel folds every row's 280 tuple bytes into
 * a 64-bit key, the host groups the keys (truncated to lcv_debug_dedup_hash_bits' bits) and a second kernel compares
 * every row but a group's first with that first row in full; groups whose members differ are split and compared again
 * (one launch per extra distinct content under one key value).  Rows merge only on a full compare.  The batch then
 * keeps the column on the host (with signature_slot, and store_index where it carries one: one device-to-host copy
 * each), and every later validation with the mode on groups it as an uploaded batch.  *classes_out: the number of
 * distinct classes.  Classifying again yields the same column.  A batch of no rows: LCV_OK, 0 classes.  A null argument:
 * LCV_EINVAL.  Synchronous, on work-space slot 0's stream: wait for pending slots first.  Device scratch: 20 bytes per
 * row of a chunk (lcv_debug_set_chunk), freed on return; longer batches take one launch per chunk of rows or pairs.
 * lcv_last_classify_timings: kernel time of the last classify, [0] the keys, [1] the compares; not stages of
 * lcv_last_timings, which reads all zero after a classify.
 * lcv_debug_batch_classes (test hook): the n class labels of a batch; LCV_EINVAL for a batch that has none.
 * lcv_batch_fan_out makes a resident batch of n rows: row i is row rows[i] of src (each < src's n, repeats allowed;
 * rows == NULL: row i, and n must be src's n), gathered on the device as lcv_batch_download's row list is; src's whole
 * pool is copied device to device, so nsc_index stays valid.  store_index != NULL: the result is a table batch with that
 * column, as lcv_batch_upload_stores makes (checked against the table at validation time, not here); NULL: a
 * single-store batch.  The classes of a classed src are inherited on the host (cls[i] = src's cls[rows[i]]: equal
 * labels, equal tuples); the result of an unclassed src is unclassed.  Refused with LCV_EINVAL before any launch,
 * lcv_last_error naming the first offender, *out = NULL: a null ctx, src or out; rows and store_index both NULL; n == 0
 * or n >= 2^32 - 1; rows[i] >= src's n.  Synchronous, on slot 0's stream; freed by lcv_batch_free.
 * The asynchronous form of this path on the eight slots, for the gossip kinds: lcv_relay_async, below.
 * Out of scope: classing inside lcv_batch_decode or lcv_create_updates_resident by default; merging across chunks;
 * bootstraps. */
int lcv_batch_classify(lcv_ctx* ctx, lcv_dbatch* b, uint64_t* classes_out);
int lcv_last_classify_timings(lcv_ctx* ctx, float ms_out[2]);
int lcv_debug_batch_classes(lcv_ctx* ctx, const lcv_dbatch* b, uint32_t* out /* n */);
int lcv_batch_fan_out(lcv_ctx* ctx, lcv_dbatch* src, const uint32_t* rows, const uint32_t* store_index, uint64_t n,
                      lcv_dbatch** out);

/* ---- Batch verification: one final exponentiation per group of rows (randomised linear combination, as blst's
 * verify_multiple_aggregate_signatures).  For a group of G consecutive items of a chunk (the rows; under
 * lcv_set_dedup the distinct items; the last group may be short) and secret 64-bit coefficients r_i,
 *     prod_i  e(r_i PK_i, H(m_i)) e(r_i (-G1), S_i)  ==  1
 * holds when every item of the group is valid, and fails when one is not except with probability about 2^-64.  So a
 * group pays ONE final exponentiation; the items of a failing group then pay one each, over their own scaled Miller
 * value (e(PK_i, H_i) e(-G1, S_i))^r_i, which is 1 exactly when the unscaled one is (0 < r_i < the group order, all
 * points in the prime-order subgroups): the fallback is exact.  Worst case, every group failing: (1 + 1/G) final
 * exponentiations per item, plus the scaling.
 * lcv_set_rlc(ctx, group, seed32): group 0 turns the mode off (the default: every call then launches exactly what it
 * launches without this entry); group in {2, 4, 8, 16, 32, 64} turns it on.  Any other value, or a missing or all-zero
 * seed with group != 0, is LCV_EINVAL; so is the mode together with a multi-stream pipeline (lcv_set_pipeline
 * streams > 1), from whichever call comes second (the sliced chains are not taught the mode).
 * Coefficients: r_i = the first 8 bytes, read little-endian, of SHA-256(seed32 || counter || i), 0 replaced by 1;
 * counter is a u64 (little-endian) per context that every chunk running the mode takes and increments, i the item's
 * index in its chunk as a u32 (little-endian).  They are derived on the device.
 * Security conditions.  The seed must be unpredictable to whoever supplies updates (draw it from the system's
 * random source; one who knows the coefficients can build invalid rows whose group product is 1).  Coefficients never
 * repeat across batches of a context (the counter); use a fresh seed per context.  The mode accepts a group
 * wrongly with probability at most about 2^-64 per group; every other accept / reject, and every reason byte, is that
 * of the mode off.  The product relies on: participant keys KeyValidated (lcv_set_store*); the signature's G2
 * membership, checked by its line walk before the product reads the flag; H(m) cofactor-cleared.  An item failing one
 * of these — no aggregate key, an undecodable signature or one outside G2 — or, where the items are the rows, a
 * pre-check is excluded from its group, never multiplied in, and never retried.
 * Scope: chunks on the batch engine; a chunk the fan engine takes (lcv_set_latency_mode) runs as with the mode off and
 * counts no groups, as does every chunk in the CPU-baseline build.  Every validate entry is covered (staged, resident,
 * asynchronous, store tables, the folds, sharded); lcv_fast_aggregate_verify* is not.  Scratch: one allocation per
 * work-space slot, made by the slot's first call with the mode on (1.35 KB per row of the slot's capacity).
 * lcv_last_rlc: the groups and the rows retried after a failing group, totals over the chunks of the last batch
 * enqueued on `slot` (synchronous calls: slot 0); valid once that batch has been waited for; it does a small
 * blocking device-to-host read of its own.  groups == 0: the mode did not act.
 * Test hooks: lcv_debug_rlc_coeffs writes the n coefficients the device derives for batch counter `counter` under the
 * seed of the last lcv_set_rlc; lcv_debug_rlc_scale writes r_i P_i (affine x || y, 48 big-endian bytes each, as p96)
 * through the scaling kernel's ladder and shared inversion.
 * Out of scope: one signature Miller loop per group (aggregating the signatures in G2); bisecting a failing group;
 * groups across chunks or batches; the sliced pipeline. */
int lcv_set_rlc(lcv_ctx* ctx, uint32_t group, const uint8_t seed32[32]);
int lcv_last_rlc(lcv_ctx* ctx, int slot, uint64_t* groups, uint64_t* retried_rows);
int lcv_debug_rlc_coeffs(lcv_ctx* ctx, uint64_t counter, uint64_t n, uint64_t* out_u64);
int lcv_debug_rlc_scale(lcv_ctx* ctx, const uint8_t* p96, const uint64_t* r_u64, uint64_t n, uint8_t* out96);
/* kernel time of the last validate call: total and per stage (ms); names via lcv_stage_name
 * (stage times are recorded by the serial shape only: zero under a multi-stream pipeline) */
int lcv_last_timings(lcv_ctx* ctx, float* ms_out, int max_stages, int* nstages);
const char* lcv_stage_name(int stage);

/* ---- multi-GPU: one process and one context per GPU, updates sharded by contiguous
 * index range, RCCL over xGMI for the one collective (the per-update verdict all-gather).  No reference
 * counterpart: the reference is single-process (p2p-interface.md:69,99 is the ingress producing batches).
 * lcv_comm_unique_id: rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to every rank. */
int lcv_comm_unique_id(uint8_t* id128);
int lcv_comm_init(lcv_ctx* ctx, int nranks, int rank, const uint8_t* id128);
int lcv_comm_destroy(lcv_ctx* ctx);
/* ranks in the communicator as RCCL reports them (ncclCommCount) */
int lcv_comm_count(lcv_ctx* ctx, int* nranks_out);
/* validate this rank's resident shard (n <= per_rank), all-gather every rank's per_rank verdict bytes
 * (zero padded) into verdict_all_out (nranks * per_rank bytes, rank-major) */
int lcv_validate_sharded(lcv_ctx* ctx, lcv_dbatch* b, uint64_t current_slot, const uint8_t* genesis_validators_root,
                         uint64_t per_rank, uint8_t* verdict_all_out);
/* max over ranks of one double (in place); doubles as a barrier */
int lcv_comm_allreduce_max(lcv_ctx* ctx, double* inout);
/* Failure containment (a failed GPU's shard is re-run).  Every collective completes within
 * the communicator timeout (default 60 s) or the call fails with LCV_EDEVICE: the wait polls the stream and
 * RCCL's asynchronous error (ncclCommGetAsyncError), so a rank whose peer died or hangs returns instead of
 * blocking in ncclAllGather.  The communicator is then marked failed (collectives refused, LCV_ESTATE) until
 * the surviving ranks all call lcv_comm_shrink with the same list of excluded ranks (ncclCommShrink with
 * NCCL_SHRINK_ABORT: the failed parent's operations are terminated, the survivors renumbered in rank
 * order; new_rank / new_nranks out), or lcv_comm_abort (ncclCommAbort) drops it. */
int lcv_comm_set_timeout(lcv_ctx* ctx, double seconds);
int lcv_comm_shrink(lcv_ctx* ctx, const int* exclude_ranks, int nexclude, int* new_rank, int* new_nranks);
int lcv_comm_abort(lcv_ctx* ctx);

/* ---- bls.FastAggregateVerify (sync-protocol.md:464); py_ecc semantics (every key KeyValidated).
 * Any number of pubkeys (npk = 0 -> False), a message of any length (the light-client call site passes
 * a 32-byte signing root; other lengths take the device's byte-streamed expand_message_xmd). */
int lcv_fast_aggregate_verify(lcv_ctx* ctx, const uint8_t* pubkeys48, uint64_t npk, const uint8_t* msg,
                              uint64_t msg_len, const uint8_t* sig96, int* result);
/* batched: committee table (ncomm x 512 x 48 B), per item committee id + participation bits */
int lcv_fast_aggregate_verify_batch(lcv_ctx* ctx, const uint8_t* committees, uint64_t ncomm,
                                    const uint32_t* committee_id, const uint8_t* bits64, const uint8_t* msg32,
                                    const uint8_t* sig96, uint64_t n, uint8_t* verdict_out);

/* ---- SSZ */
int lcv_merkle_branch_batch(lcv_ctx* ctx, const uint8_t* leaf32, const uint8_t* branch, uint32_t depth,
                            uint64_t index, const uint8_t* root32, uint64_t n, uint8_t* out);
int lcv_htr_sync_committee_batch(lcv_ctx* ctx, const uint8_t* committees, uint64_t n, uint8_t* roots32_out);
/* initialize_light_client_store's asserts (sync-protocol.md:353-362), one bootstrap per row (header rows
 * as lcv_header_cols, committee 24624 B, current_sync_committee_branch 5 x 32 B, trusted_block_root 32 B):
 * reason 0 ok, 1 header invalid (:353), 2 beacon root != trusted root (:354), 3 committee branch (:356) */
int lcv_bootstrap_check_batch(lcv_ctx* ctx, const uint8_t* beacon112, const uint8_t* exec832,
                              const uint8_t* exec_branch128, const uint8_t* committees, const uint8_t* committee_branch160,
                              const uint8_t* trusted_root32, uint64_t n, uint8_t* reason_out);

/* ---- the producer side, batched (full-node.md: create_light_client_update :138-188, _finality_update :197-205,
 * _optimistic_update :213-219, create_light_client_bootstrap :105-121; block_to_light_client_header :43-91).
 * Input: tables of sparse views and, per update, rows of those tables — a view shared by many updates (a block is
 * `block` of one update and `attested_block` of the next) is hashed once.  A state view keeps the five fields the
 * light-client data reads and every BeaconState field by its hash_tree_root (field_roots, 28 x 32 B in field
 * order; entries 2, 4, 20, 22, 23 are recomputed); its two committees are rows of `committees` (ncomm x 24624 B,
 * the distinct SSZ SyncCommittee values).  A block view keeps the header fields, the sync aggregate, the payload
 * as the 832-byte execution record above and every body field by root (body_roots, 12 x 32 B; entry 8 is
 * recomputed, entry 9 when exec_kind != 0).  exec_kind: 0 no payload, 1 Capella (15 fields), 2 Deneb (17).
 * Every index — the cases', cur_index / nxt_index — and exec_kind are checked on the host before anything is
 * launched: LCV_EINVAL names the first offender, no kernel runs and reason_out is not written.
 * Kernels (lcv_last_timings: produce_views, produce_rows): HTR(SyncCommittee) per committee row; per block view the
 * body tree -> header, block root, execution branch; per state view the state tree -> state root, the three
 * branches, the root of latest_block_header with that state root; then per update the asserts and the row.
 * reason_out[i] (lcv_producer_reason): the k-th check of create_light_client_update in evaluation order, the first
 * failing one.  A row with a non-zero reason is LightClientUpdate(): every column zero, nsc_index = ncomm.
 * Output pool: the ncomm input rows, then one all-zero row (npool = ncomm + 1); nsc_index[i] is the attested
 * state's nxt_index where the update carries a next_sync_committee, else ncomm.  kind: 0 update, 1 finality update
 * (next-committee fields zero), 2 optimistic update (finalized fields zero too), as lcv_ssz_decode_updates' rows.
 * The fork epochs and periods are lcv_set_config's.  n == 0: LCV_OK, nothing done (*out = NULL). */
enum lcv_producer_reason {
  LCV_P_OK = 0,
  LCV_P_ATTESTED_PRE_ALTAIR = 1,    /* :143 */
  LCV_P_NO_PARTICIPANTS = 2,        /* :144 */
  LCV_P_STATE_SLOT = 3,             /* :146 state.slot != state.latest_block_header.slot */
  LCV_P_STATE_BLOCK = 4,            /* :149 header root (state_root filled in) != hash_tree_root(block.message) */
  LCV_P_ATTESTED_STATE_SLOT = 5,    /* :152 */
  LCV_P_ATTESTED_BLOCK = 6,         /* :155 attested header root, attested block root, block.parent_root */
  LCV_P_ATTESTED_NO_PAYLOAD = 7,    /* :160 attested block at a Capella-or-later epoch with exec_kind 0 */
  LCV_P_FINALIZED_NO_PAYLOAD = 8,   /* :171 the same for the finalized block */
  LCV_P_FINALIZED_ROOT = 9,         /* :172 finalized header root != attested_state.finalized_checkpoint.root */
  LCV_P_FINALIZED_GENESIS = 10      /* :174 genesis finalized block, checkpoint root not zero */
};
typedef struct lcv_state_views {
  const uint64_t* slot;                /* ns */
  const uint8_t* latest_block_header;  /* ns x 112 */
  const uint64_t* fin_epoch;           /* ns: finalized_checkpoint.epoch */
  const uint8_t* fin_root;             /* ns x 32: finalized_checkpoint.root */
  const uint8_t* field_roots;          /* ns x 28 x 32 */
  const uint32_t* cur_index;           /* ns: committee row of current_sync_committee */
  const uint32_t* nxt_index;           /* ns: committee row of next_sync_committee */
} lcv_state_views;
typedef struct lcv_block_views {
  const uint64_t* slot;            /* nb */
  const uint64_t* proposer_index;  /* nb */
  const uint8_t* parent_root;      /* nb x 32 */
  const uint8_t* state_root;       /* nb x 32 */
  const uint8_t* bits;             /* nb x 64: sync_aggregate.sync_committee_bits */
  const uint8_t* signature;        /* nb x 96 */
  const uint8_t* execution;        /* nb x 832 */
  const uint8_t* exec_kind;        /* nb */
  const uint8_t* body_roots;       /* nb x 12 x 32 */
} lcv_block_views;
typedef struct lcv_update_cases {
  const uint32_t* state;           /* n: rows of the state views */
  const uint32_t* block;           /* n: rows of the block views */
  const uint32_t* attested_state;
  const uint32_t* attested_block;
  const int32_t* finalized_block;  /* n: row of the block views, or -1: none */
} lcv_update_cases;
/* the batch is made on the device, in lcv_batch_upload's layout: every resident entry takes it; lcv_batch_free */
int lcv_create_updates_resident(lcv_ctx* ctx, const lcv_state_views* states, uint64_t ns, const lcv_block_views* blocks,
                                uint64_t nb, const uint8_t* committees, uint64_t ncomm, const lcv_update_cases* cases,
                                uint64_t n, int kind, uint8_t* reason_out, lcv_dbatch** out);
/* the same, copied out: `out` names caller-allocated columns of n rows (written through) and a pool of ncomm + 1
 * rows; out->n and out->npool are not read */
int lcv_create_updates(lcv_ctx* ctx, const lcv_state_views* states, uint64_t ns, const lcv_block_views* blocks,
                       uint64_t nb, const uint8_t* committees, uint64_t ncomm, const lcv_update_cases* cases,
                       uint64_t n, int kind, const lcv_update_batch* out, uint8_t* reason_out);
/* a resident batch back to the host: all its rows (rows == NULL, nrows ignored), or rows[0 .. nrows) in that order
 * (each < the batch's n; gathered on the device); the pool is copied whole (out->nsc_pool: the batch's npool rows) */
int lcv_batch_download(lcv_ctx* ctx, lcv_dbatch* b, const uint32_t* rows, uint64_t nrows, const lcv_update_batch* out);
/* lcv_rank_updates over a resident batch: the same kernel, the same records */
int lcv_rank_resident(lcv_ctx* ctx, lcv_dbatch* b, uint8_t* rank_out /* n x 32 */);
/* create_light_client_bootstrap per (state_idx[i], block_idx[i]), from the same view kernels, as the columns
 * lcv_bootstrap_check_batch takes; the committee as committee_index[i] = the state's cur_index.  reason: 1 :107
 * state before Altair, 2 :109 state.slot != its header's slot, 3 :112 header root != block root, 4 a Capella-or-
 * later block with exec_kind 0; such a row is all zero and its committee_index is ncomm */
int lcv_create_bootstraps(lcv_ctx* ctx, const lcv_state_views* states, uint64_t ns, const lcv_block_views* blocks,
                          uint64_t nb, const uint8_t* committees, uint64_t ncomm, const uint32_t* state_idx,
                          const uint32_t* block_idx, uint64_t n, uint8_t* beacon112, uint8_t* exec832,
                          uint8_t* exec_branch128, uint32_t* committee_index, uint8_t* committee_branch160,
                          uint8_t* reason_out);

/* ---- SSZ wire bytes of a resident batch, encoded on the device (csrc/lcv_wire_enc.hpp): what a full node serves —
 * LightClientUpdatesByRange chunks, the finality / optimistic gossip topics and their Req/Resp forms
 * (p2p-interface.md:74-115, 177-200, 222-262).  kind: 0 LightClientUpdate, 1 LightClientFinalityUpdate,
 * 2 LightClientOptimisticUpdate of the row.  The bytes are those of lcv.wire.encode_updates (the inverse of
 * lcv_ssz_decode_updates for rows that came from such messages).
 * lcv_encode_pitch: the bytes between consecutive messages of the output, a multiple of 16: the longest message of
 * `kind` over the three forks, rounded up.  kind 0 update: 26880, 1 finality: 2096, 2 optimistic: 1040; 0 for any
 * other kind.
 * lcv_batch_encode.  rows == NULL: every row of b in order (nrows ignored); else rows[0 .. nrows), each < b's n,
 * repeats allowed, gathered on the device as lcv_batch_download does.  fork: 0 Deneb, 1 Capella, 2 Altair for every
 * row, or LCV_FORK_AUTO: per row from compute_epoch_at_slot(attested beacon slot) under lcv_set_config's fork epochs
 * (>= DENEB 0, >= CAPELLA 1, else 2), so one by-range response may straddle a fork boundary (p2p-interface.md:189).
 * With m the number of messages and pitch = lcv_encode_pitch of the kind:
 *   out         m x pitch bytes, message i at out + i * pitch, EVERY byte of the m x pitch written (zero past len)
 *   len_out     m x u32: the message's length
 *   fork_out    m x u8: the fork code used
 *   version_out m x 4 B: compute_fork_version(the attested slot's epoch) — the chunk's ForkDigest context version,
 *               whatever `fork` forces
 *   status_out  m x u8: 0 ok; 1 an Altair-format row with execution data (a non-zero byte in the execution record or
 *               execution branch of a header that is encoded: the finalized header is not, for kind 2); 2 an encoded
 *               header's extra_data length > 32.  Such a row has len 0 and an all-zero area.
 * Refused with LCV_EINVAL before any launch, naming the first offender, the outputs untouched: a null argument, kind
 * or fork out of range, rows[i] >= n.  No message (b's n == 0, or rows with nrows == 0): LCV_OK, nothing written.
 * Device scratch for the areas is bounded by LCV_ENCODE_SCRATCH_BYTES, not by m: the rows are encoded in chunks of
 * LCV_ENCODE_SCRATCH_BYTES / pitch messages (2496 updates), each chunk copied out before the scratch is reused; the
 * scratch is kept by the context.  Kernel time: lcv_last_timings' wire_encode stage.  Synchronous, on work-space
 * slot 0's stream: wait for pending slots first.
 * lcv_encode_updates is upload + encode + free for rows that live on the host.
 * lcv_debug_set_encode_chunk (test hook): rows per encode chunk, where fewer than fit the scratch bound (0: the
 * default).
 * Out of scope: bootstraps, snappy framing and the Req/Resp result byte, compact (unpitched) output. */
#define LCV_FORK_AUTO (-1)
#define LCV_ENCODE_SCRATCH_BYTES (64u << 20)
uint64_t lcv_encode_pitch(int kind);
int lcv_batch_encode(lcv_ctx* ctx, lcv_dbatch* b, const uint32_t* rows, uint64_t nrows, int kind, int fork,
                     uint8_t* out, uint32_t* len_out, uint8_t* fork_out, uint8_t* version_out, uint8_t* status_out);
int lcv_encode_updates(lcv_ctx* ctx, const lcv_update_batch* batch, int kind, int fork, uint8_t* out,
                       uint32_t* len_out, uint8_t* fork_out, uint8_t* version_out, uint8_t* status_out);
int lcv_debug_set_encode_chunk(lcv_ctx* ctx, uint64_t rows);

/* ---- SSZ wire messages decoded into a resident batch on the device (csrc/lcv_wire_dec.hpp): the ingress side of
 * the wire, so that a relay goes bytes -> resident batch -> lcv_validate_resident* -> lcv_batch_encode of the accepted
 * rows and the host never holds a row.  Message i = buf[offsets[i] .. + lengths[i]]; kind and fork codes as for
 * lcv_ssz_decode_updates below; forks == NULL: `fork` for every message; else one code per message and `fork` is
 * ignored.
 * Contract: *out is a resident batch in lcv_batch_upload's layout, taken by every resident entry and freed by
 * lcv_batch_free.  Its rows and status_out (0 ok, 1 malformed) are exactly what lcv_ssz_decode_updates (forks == NULL)
 * or lcv_ssz_decode_updates_mixed produce for the same messages: the same strict rules in the same order; status 1
 * and an all-zero row for a malformed message or a fork code outside 0..2; finality and optimistic messages become
 * the update the reference builds from them; Altair-format messages become their Capella upgrade.
 * Pool order: the pool holds the distinct next_sync_committee values by content in order of first occurrence, and
 * SyncCommittee() (all zero; also the committee of a malformed row and of kinds 1 and 2) takes a row at its first
 * use.  This is the host decoder's order whenever its sampled key does not collide; where the numbering differs,
 * pool[nsc_index] still agrees row for row.  Rows merge only on a full compare on the device; a 64-bit hash of the
 * committee, computed by the decode kernel, only picks which rows are compared.
 * Refused with LCV_EINVAL before any launch, lcv_last_error naming the first offender, *out = NULL and status_out
 * untouched: a null argument; kind or fork out of range; n > LCV_DECODE_MAX_ROWS; offsets[i] + lengths[i] > buf_len
 * (computed without wrapping); more than LCV_DECODE_MAX_BYTES of staged bytes (every length rounded up to 16, plus
 * 16).  n == 0: LCV_OK and *out = NULL.
 * The host copies the messages into a pinned buffer of the context (16-byte aligned each; messages that overlap or
 * repeat in buf are staged twice) and one DMA moves it into a device scratch; both grow on demand and are kept.
 * Synchronous, on work-space slot 0's stream: wait for pending slots first.
 * Deduplication: a batch made this way has no host bytes to class and, like lcv_create_updates_resident's, is
 * validated without deduplication under lcv_set_dedup until lcv_batch_classify has classed it on the device.
 * lcv_last_decode_timings: kernel time of the last decode, [0] the decode kernel's passes, [1] the committee
 * compares and the pool gather (0 for kinds 1 and 2).  These launches are not stages of lcv_last_timings, which
 * reads all zero after a decode.
 * lcv_debug_decode_hash_bits (test hook): the committee hash truncated to `bits` bits for the grouping (default 64;
 * 0 makes every committee collide, so that only the full compares separate them), as lcv_debug_dedup_hash_bits.
 * The asynchronous wire-in entry on the eight slots (kinds 1 and 2): lcv_relay_async, below.
 * Out of scope: decoding inside the streaming validation, bootstraps, snappy framing and the Req/Resp result byte,
 * merging pools across calls. */
#define LCV_DECODE_MAX_ROWS 65536u
#define LCV_DECODE_MAX_BYTES (2ull << 30)
int lcv_batch_decode(lcv_ctx* ctx, const uint8_t* buf, uint64_t buf_len, const uint64_t* offsets,
                     const uint64_t* lengths, uint64_t n, int kind, int fork,
                     const uint8_t* forks /* NULL, or one code per message */, uint8_t* status_out /* n */,
                     lcv_dbatch** out);
int lcv_last_decode_timings(lcv_ctx* ctx, float ms_out[2]);
int lcv_debug_decode_hash_bits(lcv_ctx* ctx, uint32_t bits);

/* ---- The asynchronous relay: wire messages to per-store verdicts on the eight slots (gossip kinds: 1 finality,
 * 2 optimistic).  lcv_relay_async stages the messages and the (message, store) pair list into work-space slot `slot`,
 * enqueues decode, fan-out, validation against the store table and, with fold_in, the segmented fold, and returns
 * without waiting; lcv_slot_wait_relay waits and hands out the statuses, verdicts, reasons and fold results.  Nothing
 * blocks on the device between the two, and nothing is allocated per call once the slot's buffers have grown.
 * Contract: status_out[j] is exactly lcv_batch_decode's status of message j.  Pair i's verdict and reason are exactly
 * those of lcv_batch_decode of the messages, lcv_batch_fan_out(rows, store_index) of that batch and
 * lcv_validate_resident of the result under the store table that is set when lcv_relay_async is called: byte for
 * byte with lcv_set_dedup off or on and lcv_set_rlc off or on (with it on: up to the documented 2^-64).  A malformed
 * message is an all-zero row and its pairs keep that row's verdict and reason.  With fold_in (nstore entries, as
 * lcv_validate_stores_async_fold's `in`) fold_out[s] is exactly lcv_validate_stores_fold's result for the host batch
 * of the same rows and the same store_index; entries of stores without a pair are left untouched.
 * How: one pinned region of the slot takes the messages (16-byte aligned each, 16 zero bytes behind the last), the
 * per-message (offset, length, fork), the rows and store_index columns and, with lcv_set_dedup on, the grouping into
 * BLS items, with fold_in the grouping by store and the present stores' states; ONE DMA moves it.  One kernel
 * (F_wire_relay, csrc/lcv_wire_dec.hpp) decodes message rows[i] straight into row i of the slot's table batch, one
 * 64-lane team per pair, and writes one status record per message with a team of its own; the validation follows in
 * stream order.  With lcv_set_dedup on, the host reads the class tuple of every message where it lies (the host
 * decoder's walk) and groups the pairs by (class of the message, committee row of the store) before the copy:
 * lcv_last_dedup(slot) reports what the synchronous path reports for the same input.  With the mode off the host
 * parses nothing.
 * Refused before anything is staged or launched, LCV_EINVAL with lcv_last_error naming the first offender: a null
 * argument; slot not in 0..7; kind not 1 or 2 (0, the full update, needs a device round trip for its committee pool:
 * the synchronous path serves it); fork out of range with forks == NULL; nmsg == 0 or npairs == 0; nmsg >
 * LCV_DECODE_MAX_ROWS; npairs above the chunk size (65536; lcv_debug_set_chunk); offsets[j] + lengths[j] > buf_len
 * (computed without wrapping); staged bytes above LCV_RELAY_MAX_BYTES; rows[i] >= nmsg; store_index[i] >= nstore; a
 * present fold_in[s] whose maxima exceed 512; a multi-stream pipeline (lcv_set_pipeline streams > 1).  No store table
 * set: LCV_ESTATE.
 * lcv_slot_wait_relay: LCV_ESTATE for a slot whose last batch was not a relay, and for fold_out != NULL on a relay
 * enqueued without fold_in; any out pointer may be NULL.  lcv_slot_wait on a relay slot hands out the verdicts and
 * reasons as for any staged batch; lcv_slot_wait_fold and lcv_slot_wait_stores_fold return LCV_ESTATE there.
 * Ordering: as lcv_validate_stores_async — the caller's buffers are free when the call returns; a relay and any other
 * staged or resident batch may be in flight on different slots; lcv_set_store_table waits for all slots.
 * lcv_last_relay_timings: [0] the device time of the slot's last decode + fan-out kernel (waits for it), [1] 0.
 * Out of scope: kind 0; merging classes across batches in flight; a sharded relay; snappy framing and the Req/Resp
 * result byte; bootstraps; applying the fold's result to the store table on the device. */
#define LCV_RELAY_MAX_BYTES (256ull << 20) /* staged message bytes, each length rounded up to 16, plus 16 */
typedef struct lcv_relay_request {
  const uint8_t* buf;
  uint64_t buf_len;
  const uint64_t* offsets; /* message j = buf[offsets[j] .. + lengths[j]) */
  const uint64_t* lengths;
  uint64_t nmsg;
  int kind;                /* 1 finality, 2 optimistic; 0 (update) is refused */
  int fork;                /* as lcv_batch_decode: forks == NULL -> `fork` for every message */
  const uint8_t* forks;
  const uint32_t* rows;        /* npairs: message of pair i */
  const uint32_t* store_index; /* npairs: store-table row of pair i */
  uint64_t npairs;
  uint64_t current_slot;
  const uint8_t* genesis_validators_root;
  const lcv_fold_state* fold_in; /* NULL: no fold; else nstore entries */
} lcv_relay_request;
int lcv_relay_async(lcv_ctx* ctx, const lcv_relay_request* rq, int slot);
int lcv_slot_wait_relay(lcv_ctx* ctx, int slot, uint8_t* status_out /* nmsg */, uint8_t* verdict_out /* npairs */,
                        uint8_t* reason_out /* npairs */, lcv_fold_result* fold_out /* nstore, or NULL */);
int lcv_last_relay_timings(lcv_ctx* ctx, int slot, float ms_out[2]);

/* ---- SSZ wire decode (host only, no device work; csrc/lcv_wire.cpp).  Replaces the upstream SSZ
 * deserialisation of the reference's containers (sync-protocol.md:109-115 LightClientBootstrap,
 * :120-133 LightClientUpdate, :138-148 LightClientFinalityUpdate, :153-160 LightClientOptimisticUpdate)
 * as received over Req/Resp / gossip (p2p-interface.md).  kind: 0 update, 1 finality update,
 * 2 optimistic update (converted as sync-protocol.md:563-571 / :582-590 do); fork: 0 Deneb
 * ExecutionPayloadHeader (17 fields), 1 Capella (15), 2 Altair (LightClientHeader = beacon only; the
 * row is its Capella upgrade: empty execution and branch).  Message i = buf[offsets[i] .. + lengths[i]] ->
 * row i of `out` (caller-allocated columns of n rows; out->nsc_pool is ignored).  status[i] = 0 ok,
 * 1 malformed (row zeroed).  Distinct next_sync_committee values: pool row k is the committee at
 * buf + pool_src[k] (UINT64_MAX = SyncCommittee()), *npool_out rows (<= n + 1). */
int lcv_ssz_decode_updates(const uint8_t* buf, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                           int kind, int fork, const lcv_update_batch* out, uint64_t* pool_src,
                           uint64_t* npool_out, uint8_t* status);
/* the same with a fork per message (a Req/Resp response's chunks each carry their own ForkDigest
 * context, p2p-interface.md:189-200, so one response may straddle a fork boundary) */
int lcv_ssz_decode_updates_mixed(const uint8_t* buf, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                                 int kind, const uint8_t* forks, const lcv_update_batch* out, uint64_t* pool_src,
                                 uint64_t* npool_out, uint8_t* status);
int lcv_ssz_decode_bootstrap(const uint8_t* buf, uint64_t len, int fork, uint8_t* beacon112, uint8_t* exec832,
                             uint8_t* exec_branch128, uint8_t* committee24624, uint8_t* committee_branch160,
                             uint8_t* status);

/* ---- synthetic-data signer (producer side).  Secret keys 32 B big-endian. */
int lcv_sk_to_pk_batch(lcv_ctx* ctx, const uint8_t* sk32, uint64_t n, uint8_t* pk48_out);
int lcv_sign_batch(lcv_ctx* ctx, const uint8_t* sk32, const uint8_t* msg32, uint64_t n, uint8_t* sig96_out);

/* ---- parity-test entry points (intermediate values, canonical big-endian bytes) */
/* field ops on (a, b) < p: out per item = a*b, a+b, a-b, a^-1, sqrt_fp2(a + b u) (2 x 48); ok = sqrt exists */
/* test hook: rows per validate chunk (1 .. 65536; default 65536) */
int lcv_debug_set_chunk(lcv_ctx* ctx, uint64_t rows);
/* test hook (host arithmetic only): allocates work-space slots 0 .. nslots-1 for `cap` rows and checks
 * (1) for slices of `slice` rows, that item j of each slice's work view is item base + j of the slot's
 * work space in every per-item field, element for element, as the kernels address them, and (2) that the
 * byte ranges of every field of every slot — the committee-pool fields (HTR roots and flags of a pool of 5
 * distinct committees) included — are pairwise disjoint.  LCV_EINVAL + lcv_last_error names the first
 * field that fails. */
int lcv_debug_work_check(lcv_ctx* ctx, uint64_t cap, uint64_t slice, int nslots);
/* test hook (device backend): hold work-space slot `slot`'s main stream with a kernel that waits for
 * lcv_debug_release_slots or max_seconds (<= 120), so that a collective behind it cannot complete */
int lcv_debug_hold_slot(lcv_ctx* ctx, int slot, double max_seconds);
int lcv_debug_release_slots(lcv_ctx* ctx);
/* build provenance: a hash of the sources liblcv.so was compiled from (tools/build_id.py: csrc/, include/,
 * tools/gen_sop.py, the Makefile), NUL-terminated into out (cap >= 17); LCV_EINVAL if cap is too small */
int lcv_build_id(char* out, uint64_t cap);
/* test hook: HIP events held by the context's stage-timing pool (bounded under asynchronous calls) */
int lcv_debug_event_pool(lcv_ctx* ctx, uint64_t* events_out);
int lcv_debug_fp(lcv_ctx* ctx, const uint8_t* a48, const uint8_t* b48, uint64_t n, uint8_t* out288, uint8_t* ok);
/* a^((p+1)/4) || a^((p-3)/4) (2 x 48 B) for a < p: the windowed sqrt exponentiations of decompression / SSWU */
int lcv_debug_fp_pow(lcv_ctx* ctx, const uint8_t* a48, uint64_t n, uint8_t* out96);
/* hash_to_G2(msg) affine (x0 || x1 || y0 || y1, 4 x 48 B); inf flag */
int lcv_debug_hash_to_g2(lcv_ctx* ctx, const uint8_t* msg32, uint64_t n, uint8_t* out192, uint8_t* inf);
/* signature decode + subgroup check: affine point + status (0 ok, 1 identity, 2 invalid) */
int lcv_debug_g2_decompress(lcv_ctx* ctx, const uint8_t* sig96, uint64_t n, uint8_t* out192, uint8_t* status);
/* masked aggregate (affine x || y) + status (0 ok, 1 identity, 2 invalid key among participants) */
int lcv_debug_aggregate(lcv_ctx* ctx, const uint8_t* committees, uint64_t ncomm, const uint32_t* committee_id,
                        const uint8_t* bits64, uint64_t n, uint8_t* out96, uint8_t* status);
/* e(P, Q)^3 after final exponentiation (12 x 48 B, coefficient order g0..g5 of w^i, each c0 || c1) */
int lcv_debug_pairing(lcv_ctx* ctx, const uint8_t* p96, const uint8_t* q192, uint64_t n, uint8_t* out576);

#ifdef __cplusplus
}
#endif
#endif /* LCV_H */
