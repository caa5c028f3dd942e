"""Light-client store state machine over GPU-verified batches.

Host restatement of the reference's store logic, driven by the batched HIP verifier:

    get_safety_threshold                    sync-protocol.md:323-327
    is_better_update                        sync-protocol.md:260-311
    apply_light_client_update               sync-protocol.md:470-486
    process_light_client_store_force_update sync-protocol.md:490-503
    process_light_client_update             sync-protocol.md:508-553
    process_light_client_finality_update    sync-protocol.md:559-573
    process_light_client_optimistic_update  sync-protocol.md:578-592
    initialize_light_client_store           sync-protocol.md:351-373 (its three asserts run in the
                                            HIP kernel F_bootstrap)

plus `process_light_client_updates(store, updates, current_slot, gvr)`: the reference's sequential
loop `for u in updates: process_light_client_update(store, u, ...)` (an AssertionError rejects the
update and leaves the store unchanged: validation runs before any mutation), returning the accept
flags.  Validation is speculative and batched: every pending update is validated on the GPU against
the current store snapshot in ONE call; the host then applies the store logic in order, and only
when `apply_light_client_update` changes what validation reads (finalized slot, current / next
sync committee) are the remaining updates re-validated, again as one batch.  The store mutation
itself is scalar and order-dependent, so it stays on the host.

`sync_light_client_updates` is the same loop for the case where (nearly) every update moves the store —
catching up over sync-committee periods, one LightClientUpdate per period (light-client.md step 4.2,
p2p-interface.md LightClientUpdatesByRange): the store each update will meet is predicted on the host and all
updates are validated in one device call, each against its own predicted store (the store table).

Store / update objects are duck-typed: any objects with the reference's field names (the spec
containers, or the lightweight defaults below for the finality / optimistic conversions).
"""
from __future__ import annotations

import copy
import hashlib
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Optional, Sequence

import numpy as np

from . import config
from . import layout as L
from . import runtime
from ._native import FOLD_MAX_ROWS, STORE_NEXT_UNKNOWN
from .device import (FoldState, PackedUpdates, RANK_DTYPE, RANK_FIN, RANK_FIN_SC, RANK_REL_SC, RANK_SUPER, ResidentBatch,
                     Verifier)
from .sync_protocol import REASONS, pack_updates, validate_light_client_updates, validate_under_store_keys

# SLOTS_PER_EPOCH * EPOCHS_PER_SYNC_COMMITTEE_PERIOD and UPDATE_TIMEOUT (sync-protocol.md:89) come from the
# active network configuration (lcv.config.active(); mainnet unless set)


# ------------------------------------------------------------------ predicates (sync-protocol.md:246-341)
def _zero(b: bytes) -> bool:
    return not any(b)


def compute_sync_committee_period_at_slot(slot) -> int:
    return config.active().compute_sync_committee_period_at_slot(slot)


def is_sync_committee_update(update) -> bool:
    return not _zero(L.pack_branch(update.next_sync_committee_branch, 5))


def is_finality_update(update) -> bool:
    return not _zero(L.pack_branch(update.finality_branch, 6))


def is_next_sync_committee_known(store) -> bool:
    return not _zero(L.pack_sync_committee(store.next_sync_committee))


def get_safety_threshold(store) -> int:
    return max(int(store.previous_max_active_participants), int(store.current_max_active_participants)) // 2


def _participants(update) -> int:
    return int(sum(bool(b) for b in update.sync_aggregate.sync_committee_bits))


def _slot(header) -> int:
    return int(header.beacon.slot)


# ------------------------------------------------------------------ store logic
def is_better_update(new_update, old_update) -> bool:
    """sync-protocol.md:260-311."""
    max_active = len(new_update.sync_aggregate.sync_committee_bits)
    new_n, old_n = _participants(new_update), _participants(old_update)
    new_super, old_super = new_n * 3 >= max_active * 2, old_n * 3 >= max_active * 2
    if new_super != old_super:
        return new_super > old_super
    if not new_super and new_n != old_n:
        return new_n > old_n

    def relevant_sc(u):
        return is_sync_committee_update(u) and (compute_sync_committee_period_at_slot(_slot(u.attested_header))
                                                == compute_sync_committee_period_at_slot(u.signature_slot))
    new_rel, old_rel = relevant_sc(new_update), relevant_sc(old_update)
    if new_rel != old_rel:
        return new_rel
    new_fin, old_fin = is_finality_update(new_update), is_finality_update(old_update)
    if new_fin != old_fin:
        return new_fin
    if new_fin:
        def sc_finality(u):
            return (compute_sync_committee_period_at_slot(_slot(u.finalized_header))
                    == compute_sync_committee_period_at_slot(_slot(u.attested_header)))
        new_scf, old_scf = sc_finality(new_update), sc_finality(old_update)
        if new_scf != old_scf:
            return new_scf
    if new_n != old_n:
        return new_n > old_n
    if _slot(new_update.attested_header) != _slot(old_update.attested_header):
        return _slot(new_update.attested_header) < _slot(old_update.attested_header)
    return int(new_update.signature_slot) < int(old_update.signature_slot)


def apply_light_client_update(store, update) -> None:
    """sync-protocol.md:470-486."""
    store_period = compute_sync_committee_period_at_slot(_slot(store.finalized_header))
    update_finalized_period = compute_sync_committee_period_at_slot(_slot(update.finalized_header))
    if not is_next_sync_committee_known(store):
        assert update_finalized_period == store_period
        store.next_sync_committee = update.next_sync_committee
    elif update_finalized_period == store_period + 1:
        store.current_sync_committee = store.next_sync_committee
        store.next_sync_committee = update.next_sync_committee
        store.previous_max_active_participants = store.current_max_active_participants
        store.current_max_active_participants = 0
    if _slot(update.finalized_header) > _slot(store.finalized_header):
        store.finalized_header = update.finalized_header
        if _slot(store.finalized_header) > _slot(store.optimistic_header):
            store.optimistic_header = store.finalized_header


def process_light_client_store_force_update(store, current_slot: int) -> None:
    """sync-protocol.md:490-503 (the best update's finalized header is replaced on a copy, so the
    caller's update object is not mutated)."""
    if int(current_slot) > _slot(store.finalized_header) + config.active().UPDATE_TIMEOUT and store.best_valid_update is not None:
        best = store.best_valid_update
        if _slot(best.finalized_header) <= _slot(store.finalized_header):
            best = SimpleNamespace(**{k: getattr(best, k) for k in _UPDATE_FIELDS})
            best.finalized_header = best.attested_header
        apply_light_client_update(store, best)
        store.best_valid_update = None


def _apply_valid(store, update) -> None:
    """process_light_client_update (sync-protocol.md:508-553) after validation succeeded."""
    n = _participants(update)
    if store.best_valid_update is None or is_better_update(update, store.best_valid_update):
        store.best_valid_update = update
    store.current_max_active_participants = max(int(store.current_max_active_participants), n)
    if n > get_safety_threshold(store) and _slot(update.attested_header) > _slot(store.optimistic_header):
        store.optimistic_header = update.attested_header
    has_finalized_next = (not is_next_sync_committee_known(store) and is_sync_committee_update(update)
                          and is_finality_update(update)
                          and compute_sync_committee_period_at_slot(_slot(update.finalized_header))
                          == compute_sync_committee_period_at_slot(_slot(update.attested_header)))
    if n * 3 >= len(update.sync_aggregate.sync_committee_bits) * 2 and (
            _slot(update.finalized_header) > _slot(store.finalized_header) or has_finalized_next):
        apply_light_client_update(store, update)
        store.best_valid_update = None


def _validation_key(store):
    """What validate_light_client_update reads from the store."""
    return (_slot(store.finalized_header), L.pack_sync_committee(store.current_sync_committee),
            L.pack_sync_committee(store.next_sync_committee))


def process_light_client_updates(store, updates: Sequence, current_slot: int, genesis_validators_root: bytes,
                                 verifier: Optional[Verifier] = None, reasons_out: Optional[list] = None
                                 ) -> np.ndarray:
    """Sequential `process_light_client_update` over `updates` (in order) with batched GPU
    validation; returns accept flags.  `reasons_out` (optional list) receives each update's
    validation reason code (0 = valid, REASONS in lcv.sync_protocol) under the store it met."""
    v = verifier if verifier is not None else runtime.default_verifier()
    if v.config != config.active():
        # the host-side periods / UPDATE_TIMEOUT read config.active(); the device checks read v.config
        raise ValueError(f"process_light_client_updates: the verifier validates under network configuration "
                         f"{v.config.name!r} but lcv.config.active() is {config.active().name!r}; call "
                         f"lcv.config.set_active() (or Verifier.set_config) so both sides agree")
    verifier = v
    n = len(updates)
    accepted = np.zeros(n, bool)
    reasons = np.zeros(n, np.uint8)
    start = 0
    while start < n:
        key = _validation_key(store)
        ok, rs = validate_light_client_updates(store, updates[start:], current_slot, genesis_validators_root, verifier)
        k = start
        while k < n:
            reasons[k] = rs[k - start]
            if ok[k - start]:
                accepted[k] = True
                _apply_valid(store, updates[k])
            k += 1
            if _validation_key(store) != key:
                break  # the store moved: re-validate what is left against the new snapshot
        start = k
    if reasons_out is not None:
        reasons_out.extend(int(r) for r in reasons)
    return accepted


def sync_light_client_updates(store, updates: Sequence, current_slot: int, genesis_validators_root: bytes,
                              verifier: Optional[Verifier] = None, reasons_out: Optional[list] = None,
                              stats_out: Optional[dict] = None) -> np.ndarray:
    """`process_light_client_updates` — the same accept flags, reason codes and final store — with the device
    validations of a multi-period catch-up collapsed into (normally) one.

    process_light_client_updates validates the pending updates against the store as it is and starts over
    whenever an accepted update changes what validation reads, which an update per sync-committee period does
    every time: K periods cost K store uploads and K device calls.  Here the store every pending update will meet
    is predicted instead: on a shallow copy of the store (the store logic only assigns fields) each update is
    applied as if it were valid, the copy's validation key recorded before each.  All pending updates are then
    validated in ONE call, each under its predicted key (lcv.sync_protocol.validate_under_store_keys: the store
    table).  The rows are walked in order against the real store; a row's verdict counts only if the real store's
    validation key is the one the row was validated under.  It is not after an invalid update whose acceptance
    would have moved the store: from that row on the rest is planned and validated again.

    stats_out (optional dict) receives validate_calls and rows_validated."""
    v = verifier if verifier is not None else runtime.default_verifier()
    if v.config != config.active():
        raise ValueError(f"sync_light_client_updates: the verifier validates under network configuration "
                         f"{v.config.name!r} but lcv.config.active() is {config.active().name!r}; call "
                         f"lcv.config.set_active() (or Verifier.set_config) so both sides agree")
    n = len(updates)
    accepted = np.zeros(n, bool)
    reasons = np.zeros(n, np.uint8)
    calls = rows = 0
    start = 0
    while start < n:
        sim = copy.copy(store)
        keys = []
        for u in updates[start:]:
            keys.append(_validation_key(sim))
            try:
                _apply_valid(sim, u)
            except AssertionError:
                break  # apply_light_client_update's own assert: only an invalid update gets here; plan ends with it
        pending = updates[start:start + len(keys)]
        ok, rs = validate_under_store_keys(keys, pending, current_slot, genesis_validators_root, v)
        calls += 1
        rows += len(keys)
        k = start
        while k < start + len(keys) and _validation_key(store) == keys[k - start]:
            reasons[k] = rs[k - start]
            if ok[k - start]:
                accepted[k] = True
                _apply_valid(store, updates[k])
            k += 1
        start = k  # (k > start: the first row's key is the real store's)
    if reasons_out is not None:
        reasons_out.extend(int(r) for r in reasons)
    if stats_out is not None:
        stats_out["validate_calls"] = calls
        stats_out["rows_validated"] = rows
    return accepted


# ------------------------------------------------------------------ the device fold (include/lcv.h)
def _rank_key(update) -> np.void:
    """The device's rank record (lcv.device.RANK_DTYPE) of one update object, computed on the host: the store's
    own best_valid_update enters the fold through it."""
    n = _participants(update)
    att, sig, fin = _slot(update.attested_header), int(update.signature_slot), _slot(update.finalized_header)
    is_sc, is_fin = is_sync_committee_update(update), is_finality_update(update)
    period = compute_sync_committee_period_at_slot
    key0 = (RANK_SUPER if n * 3 >= L.SYNC_COMMITTEE_SIZE * 2 else n << 13) | n
    if is_sc and period(att) == period(sig):
        key0 |= RANK_REL_SC
    if is_fin:
        key0 |= RANK_FIN
        if period(fin) == period(att):
            key0 |= RANK_FIN_SC
    return np.array([(key0, 1 if is_sc else 0, att, sig, fin)], RANK_DTYPE)[0]


def _fold_check_config(v: Verifier, who: str) -> None:
    if v.config != config.active():
        raise ValueError(f"{who}: the verifier validates under network configuration "
                         f"{v.config.name!r} but lcv.config.active() is {config.active().name!r}; call "
                         f"lcv.config.set_active() (or Verifier.set_config) so both sides agree")


def _fold_state_of(store) -> FoldState:
    """The fold state of a store: its optimistic slot, its maxima, and its best_valid_update's rank (_rank_key)."""
    state = FoldState(optimistic_slot=_slot(store.optimistic_header),
                      previous_max_active_participants=int(store.previous_max_active_participants),
                      current_max_active_participants=int(store.current_max_active_participants))
    if store.best_valid_update is not None:
        k = _rank_key(store.best_valid_update)
        state.has_best, state.best_key0 = True, int(k["key0"])
        state.best_attested_slot, state.best_signature_slot = int(k["attested_slot"]), int(k["signature_slot"])
    return state


def fold_light_client_updates(store, updates, current_slot: int, genesis_validators_root: bytes,
                              verifier: Optional[Verifier] = None, reasons_out: Optional[list] = None,
                              stats_out: Optional[dict] = None) -> np.ndarray:
    """`process_light_client_updates` — the same accept flags, reason codes and final store — with the store
    logic after validation folded on the device (Verifier.validate_fold): best update, max participants,
    optimistic header and the first row that applies come back with the verdicts, so no per-row Python remains.

    `updates`: a sequence of update objects or a PackedUpdates batch (rows the store ends up holding are rebuilt
    with lcv.layout.unpack_update).  Per segment: the store is set, the fold state built from it (the old best's
    rank by _rank_key), validate_fold run over chunks of at most 65,536 rows until one reports an apply_row, the
    store's current_max_active_participants / optimistic_header / best_valid_update written from the result's
    rows, the applying row applied with apply_light_client_update, and the next segment starts after it.

    stats_out (optional dict) receives validate_calls and segments."""
    v = verifier if verifier is not None else runtime.default_verifier()
    _fold_check_config(v, "fold_light_client_updates")
    packed = isinstance(updates, PackedUpdates)
    batch = updates if packed else pack_updates(updates)
    row = (lambda i: L.unpack_update(batch, i)) if packed else (lambda i: updates[i])
    n = batch.n
    accepted = np.zeros(n, bool)
    reasons = np.zeros(n, np.uint8)
    chunk = min(FOLD_MAX_ROWS, int(getattr(v, "chunk_rows", FOLD_MAX_ROWS)))
    calls = segments = 0
    start = 0
    while start < n:
        segments += 1
        runtime.ensure_store(v, *_validation_key(store))
        state = _fold_state_of(store)
        pos, apply_row, best_row, optimistic_row = start, -1, -1, -1
        while pos < n and apply_row < 0:
            ok, rs, res = v.validate_fold(batch.slice(pos, min(n, pos + chunk)), int(current_slot),
                                          bytes(genesis_validators_root), state)
            calls += 1
            k = res.rows_consumed
            accepted[pos:pos + k] = ok[:k]
            reasons[pos:pos + k] = rs[:k]
            if res.best_row >= 0:
                best_row = pos + res.best_row
            if res.optimistic_row >= 0:
                optimistic_row = pos + res.optimistic_row
            if res.apply_row >= 0:
                apply_row = pos + res.apply_row
            state = res.next
            pos += k
        store.current_max_active_participants = state.current_max_active_participants
        if optimistic_row >= 0:
            store.optimistic_header = row(optimistic_row).attested_header
        if apply_row >= 0:
            apply_light_client_update(store, row(apply_row))
            store.best_valid_update = None
        elif best_row >= 0:
            store.best_valid_update = row(best_row)
        start = pos
    if reasons_out is not None:
        reasons_out.extend(int(r) for r in reasons)
    if stats_out is not None:
        stats_out["validate_calls"] = calls
        stats_out["segments"] = segments
    return accepted


def _take_rows(batch: PackedUpdates, idx: np.ndarray) -> PackedUpdates:
    """Rows idx of a PackedUpdates batch (the committee pool is shared)."""
    if idx.size == batch.n:  # (idx is ascending and without repeats: the whole batch)
        return batch
    kw = {f: (getattr(batch, f) if f == "nsc_pool" else np.ascontiguousarray(getattr(batch, f)[idx]))
          for f in batch.__dataclass_fields__}
    return PackedUpdates(**kw)


def fold_light_client_updates_multi(stores: Sequence, updates, current_slot: int, genesis_validators_root: bytes,
                                    verifier: Optional[Verifier] = None, reasons_out: Optional[list] = None,
                                    stats_out: Optional[dict] = None) -> np.ndarray:
    """`process_light_client_updates` for many stores at once: stores[i] is the store OBJECT update i is for (the
    same object may repeat; the rows of different stores may interleave in any way).  For every distinct store
    object S the accept flags, reason codes and final state of S are those of
    process_light_client_updates(S, [updates[i] for i if stores[i] is S], ...) — validated and folded in one
    device call per round for all stores together (Verifier.validate_stores_fold), with no per-row Python.

    `updates`: update objects or a PackedUpdates batch (rows a store ends up holding are rebuilt with
    lcv.layout.unpack_update).  A round takes the rows still pending, in order; builds a store table with one
    store row per store object that has pending rows (committees shared by content, store rows not: stores with
    equal validation keys still fold from different states) and each store's fold state; validates and folds, in
    chunks of at most 65,536 rows, a store's `next` carried from chunk to chunk until the store applies a row;
    writes every present store from its result (maxima, optimistic header, best update — or
    apply_light_client_update and no best); and keeps the rows after a store's applying row for the next round,
    which validates them against the store as it then is.  Host work is O(stores) per round and O(1) per row.

    stats_out (optional dict) receives rounds, validate_calls and table_uploads."""
    v = verifier if verifier is not None else runtime.default_verifier()
    _fold_check_config(v, "fold_light_client_updates_multi")
    packed = isinstance(updates, PackedUpdates)
    batch = updates if packed else pack_updates(updates)
    row = (lambda i: L.unpack_update(batch, int(i))) if packed else (lambda i: updates[int(i)])
    n = batch.n
    if len(stores) != n:
        raise ValueError("need one store per update")
    accepted = np.zeros(n, bool)
    reasons = np.zeros(n, np.uint8)
    objs, ordinal = [], {}
    owner = np.zeros(n, np.int64)
    for i, s in enumerate(stores):
        k = ordinal.get(id(s))
        if k is None:
            k = ordinal[id(s)] = len(objs)
            objs.append(s)
        owner[i] = k
    chunk = min(FOLD_MAX_ROWS, int(getattr(v, "chunk_rows", FOLD_MAX_ROWS)))
    cs, gvr = int(current_slot), bytes(genesis_validators_root)
    zero = hashlib.sha256(bytes(L.SYNC_COMMITTEE_BYTES)).digest()
    rounds = calls = uploads = 0
    pending = np.arange(n)
    while pending.size:
        rounds += 1
        present, local = np.unique(owner[pending], return_inverse=True)  # store row s <-> object objs[present[s]]
        ns = present.size
        # the table: one store row per present store object, committees shared by content
        com, com_row = [], {}

        def committee_row(sc: bytes) -> int:
            d = hashlib.sha256(sc).digest()
            if d == zero:
                return STORE_NEXT_UNKNOWN
            if d not in com_row:
                com_row[d] = len(com)
                com.append(sc)
            return com_row[d]

        fin, cur, nxt = np.zeros(ns, np.uint64), np.zeros(ns, np.uint32), np.zeros(ns, np.uint32)
        states = []
        for s, k in enumerate(present.tolist()):
            f, c, x = _validation_key(objs[k])
            fin[s], cur[s], nxt[s] = f, committee_row(c), committee_row(x)
            states.append(_fold_state_of(objs[k]))
        h = hashlib.sha256(b"".join(com_row))
        h.update(fin.tobytes() + cur.tobytes() + nxt.tobytes())
        committees = np.frombuffer(b"".join(com), np.uint8).reshape(len(com), L.SYNC_COMMITTEE_BYTES)
        uploads += bool(runtime.ensure_store_table(v, h.digest(), committees, fin, cur, nxt))
        apply_row, best_row, optimistic_row = (np.full(ns, -1, np.int64) for _ in range(3))  # batch rows
        left = []
        for pos in range(0, pending.size, chunk):
            rows_ix, loc = pending[pos:pos + chunk], local[pos:pos + chunk]
            live = apply_row[loc] < 0  # a store that applied in an earlier chunk consumes nothing more this round
            if not live.all():
                left.append(rows_ix[~live])
                rows_ix, loc = rows_ix[live], loc[live]
            if not rows_ix.size:
                continue
            ok, rs, res = v.validate_stores_fold(_take_rows(batch, rows_ix), loc, cs, gvr, states)
            calls += 1
            last = np.full(ns, rows_ix.size, np.int64)  # per store: the last row of this chunk it consumed
            for s, r in enumerate(res):
                if r is None:
                    continue
                states[s] = r.next
                if r.best_row >= 0:
                    best_row[s] = rows_ix[r.best_row]
                if r.optimistic_row >= 0:
                    optimistic_row[s] = rows_ix[r.optimistic_row]
                if r.apply_row >= 0:
                    apply_row[s], last[s] = rows_ix[r.apply_row], r.apply_row
            consumed = np.arange(rows_ix.size) <= last[loc]
            accepted[rows_ix[consumed]] = ok[consumed]
            reasons[rows_ix[consumed]] = rs[consumed]
            left.append(rows_ix[~consumed])
        for s, k in enumerate(present.tolist()):
            store = objs[k]
            store.current_max_active_participants = states[s].current_max_active_participants
            if optimistic_row[s] >= 0:
                store.optimistic_header = row(optimistic_row[s]).attested_header
            if apply_row[s] >= 0:
                apply_light_client_update(store, row(apply_row[s]))
                store.best_valid_update = None
            elif best_row[s] >= 0:
                store.best_valid_update = row(best_row[s])
        pending = np.sort(np.concatenate(left)) if left else np.zeros(0, np.int64)
    if reasons_out is not None:
        reasons_out.extend(int(r) for r in reasons)
    if stats_out is not None:
        stats_out["rounds"] = rounds
        stats_out["validate_calls"] = calls
        stats_out["table_uploads"] = uploads
    return accepted


def rank_updates(updates, verifier: Optional[Verifier] = None) -> np.ndarray:
    """The device's rank records (lcv.device.RANK_DTYPE, one per update) of update objects or a PackedUpdates
    batch: is_better_update(a, b) iff (key0_a, -attested_a, -signature_a) > (key0_b, -attested_b, -signature_b)."""
    v = verifier if verifier is not None else runtime.default_verifier()
    if isinstance(updates, ResidentBatch):  # a device-resident batch is ranked where it lies
        return v.rank_resident(updates)
    return v.rank(updates if isinstance(updates, PackedUpdates) else pack_updates(updates))


def best_update_per_period(updates, verifier: Optional[Verifier] = None, rank: Optional[np.ndarray] = None) -> dict:
    """full-node.md:184-187: the best LightClientUpdate (according to is_better_update) for each sync committee
    period -> {period: row}.  A row belongs to the period of its attested header; rows whose signature_slot lies
    in another period are left out.  Per period the first arg-max of the device's rank records (one lexsort).
    `updates` may be a ResidentBatch (Verifier.create_updates_resident, upload): it is ranked on the device
    without a copy, and the rows are its rows (Verifier.download(rb, rows) fetches the winners).  `rank`: the
    batch's rank records where the caller already has them (rank_updates)."""
    v = verifier if verifier is not None else runtime.default_verifier()
    rec = rank if rank is not None else rank_updates(updates, v)
    spp = v.config.SLOTS_PER_PERIOD
    period = rec["attested_slot"] // np.uint64(spp)
    rows = np.nonzero(period == rec["signature_slot"] // np.uint64(spp))[0]
    if rows.size == 0:
        return {}
    r = rec[rows]
    order = np.lexsort((rows, r["signature_slot"], r["attested_slot"], -r["key0"].astype(np.int64), period[rows]))
    p = period[rows][order]
    first = np.concatenate(([True], p[1:] != p[:-1]))
    return {int(pp): int(rr) for pp, rr in zip(p[first], rows[order][first])}


def process_light_client_update(store, update, current_slot: int, genesis_validators_root: bytes,
                                verifier: Optional[Verifier] = None) -> None:
    """sync-protocol.md:508-553: raises AssertionError (store unchanged) on an invalid update."""
    rs: list = []
    if not process_light_client_updates(store, [update], current_slot, genesis_validators_root, verifier, rs)[0]:
        line, what = REASONS.get(rs[0], ("?", "?"))
        raise AssertionError(f"validate_light_client_update: assert {what} failed ({line}, reason {rs[0]})")


# ------------------------------------------------------------------ finality / optimistic updates
_UPDATE_FIELDS = ("attested_header", "next_sync_committee", "next_sync_committee_branch", "finalized_header",
                  "finality_branch", "sync_aggregate", "signature_slot")


def _default_sync_committee():
    return SimpleNamespace(pubkeys=[bytes(L.PUBKEY_BYTES)] * L.SYNC_COMMITTEE_SIZE, aggregate_pubkey=bytes(L.PUBKEY_BYTES))


def _default_header():
    """LightClientHeader() (all-zero beacon header, execution header and branch)."""
    beacon = SimpleNamespace(slot=0, proposer_index=0, parent_root=bytes(32), state_root=bytes(32), body_root=bytes(32))
    execution = SimpleNamespace(logs_bloom=bytes(256), extra_data=b"")
    return SimpleNamespace(beacon=beacon, execution=execution, execution_branch=[bytes(32)] * 4)


def _finality_as_update(fu):
    return SimpleNamespace(attested_header=fu.attested_header, next_sync_committee=_default_sync_committee(),
                           next_sync_committee_branch=[bytes(32)] * 5, finalized_header=fu.finalized_header,
                           finality_branch=fu.finality_branch, sync_aggregate=fu.sync_aggregate,
                           signature_slot=fu.signature_slot)


def _optimistic_as_update(ou):
    return SimpleNamespace(attested_header=ou.attested_header, next_sync_committee=_default_sync_committee(),
                           next_sync_committee_branch=[bytes(32)] * 5, finalized_header=_default_header(),
                           finality_branch=[bytes(32)] * 6, sync_aggregate=ou.sync_aggregate,
                           signature_slot=ou.signature_slot)


def process_light_client_finality_update(store, finality_update, current_slot: int, genesis_validators_root: bytes,
                                         verifier: Optional[Verifier] = None) -> None:
    """sync-protocol.md:559-573."""
    process_light_client_update(store, _finality_as_update(finality_update), current_slot, genesis_validators_root,
                                verifier)


def process_light_client_optimistic_update(store, optimistic_update, current_slot: int,
                                           genesis_validators_root: bytes, verifier: Optional[Verifier] = None) -> None:
    """sync-protocol.md:578-592."""
    process_light_client_update(store, _optimistic_as_update(optimistic_update), current_slot,
                                genesis_validators_root, verifier)


# ------------------------------------------------------------------ bootstrap (sync-protocol.md:164-179, :351-373)
@dataclass
class LightClientStore:
    """sync-protocol.md:164-179 (field names and meaning as the reference's dataclass)."""
    finalized_header: Any
    current_sync_committee: Any
    next_sync_committee: Any
    best_valid_update: Optional[Any]
    optimistic_header: Any
    previous_max_active_participants: int
    current_max_active_participants: int


BOOTSTRAP_REASONS = {
    0: ("", "valid"),
    1: ("sync-protocol.md:353", "is_valid_light_client_header(bootstrap.header)"),
    2: ("sync-protocol.md:354", "hash_tree_root(bootstrap.header.beacon) == trusted_block_root"),
    3: ("sync-protocol.md:356-362", "is_valid_merkle_branch(current_sync_committee_branch)"),
}


def initialize_light_client_store(trusted_block_root: bytes, bootstrap, verifier: Optional[Verifier] = None
                                  ) -> LightClientStore:
    """sync-protocol.md:351-373: the header-validity, trusted-root and committee-branch asserts run on the
    device (lcv_bootstrap_check_batch); raises AssertionError naming the failing assert."""
    v = verifier if verifier is not None else runtime.default_verifier()
    beacon, execution, branch = L.pack_header(bootstrap.header)
    root = bytes(trusted_block_root)
    if len(root) != 32:
        raise ValueError("trusted_block_root must be 32 bytes")
    u8 = lambda b: np.frombuffer(b, np.uint8)  # noqa: E731
    r = int(v.bootstrap_check_batch(u8(beacon), u8(execution), u8(branch),
                                    u8(L.pack_sync_committee(bootstrap.current_sync_committee)),
                                    u8(L.pack_branch(bootstrap.current_sync_committee_branch, 5)), u8(root))[0])
    if r:
        line, what = BOOTSTRAP_REASONS[r]
        raise AssertionError(f"initialize_light_client_store: assert {what} failed ({line}, reason {r})")
    return LightClientStore(finalized_header=bootstrap.header, current_sync_committee=bootstrap.current_sync_committee,
                            next_sync_committee=_default_sync_committee(), best_valid_update=None,
                            optimistic_header=bootstrap.header, previous_max_active_participants=0,
                            current_max_active_participants=0)
