"""`validate_stream`: the serving loop over a stream of host batches, several in flight.

One synchronous call validates one batch and the device idles while the host stages the next; with the
batches of up to eight work-space slots in flight, a batch's upload and the host's staging overlap the other
slots' kernels (lcv_validate_async, include/lcv.h).  This is the loop bench.py writes by hand, for any caller:
single-store batches (Verifier.set_store) and table batches (Verifier.set_store_table, one store row per
update) may be mixed in one stream.

`relay_updates`: the relay's path with every row kept on the device — wire messages decoded, classed and fanned out
to the stores of many clients, validated with each distinct signature checked once.

`relay_stream`: the serving loop over that path for gossip messages, several items in flight (lcv_relay_async): one
call per item stages the bytes and the pair list and enqueues decode, fan-out and validation on a slot.
"""
from __future__ import annotations

from collections import deque
from typing import Iterable, Iterator, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from .device import FoldState, PackedUpdates, ResidentBatch, Verifier

SLOTS = 8            # work-space slots of a context (LCV_SLOTS)
MAX_ROWS = 65536     # rows of one asynchronous call

Item = Union[PackedUpdates, Tuple[PackedUpdates, np.ndarray]]


def validate_stream(verifier: Verifier, items: Iterable[Item], current_slot: int, genesis_validators_root: bytes,
                    in_flight: int = SLOTS, dedup: Optional[bool] = None,
                    rlc_group: int = 0) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
    """Validate every item of `items` and yield its (verdicts: bool array, reason codes: uint8 array), in input
    order.  An item is a PackedUpdates — validated against the store of Verifier.set_store, as
    Verifier.validate does — or (PackedUpdates, store_index) — update i against row store_index[i] of the table
    of Verifier.set_store_table, as Verifier.validate_stores does.  The store and the table an item needs must
    be set before the item is drawn from `items`; a set_store_table between two items waits for the items in
    flight, which finish under the table they were enqueued under.

    Up to `in_flight` (1..8) calls are in flight, on work-space slots 0 .. in_flight - 1 in turn, through
    Verifier.validate_async / validate_stores_async; the generator waits for a slot only when it is about to
    reuse it (and, after the last item, for what is left).  Items above 65,536 rows — the rows of one
    asynchronous call — are cut into pieces, and an item's result is yielded whole.  No other call may use the
    verifier's slots while the generator is live; closing it early waits for the slots in flight.

    `dedup`: None leaves the verifier's setting (Verifier.set_dedup) alone; a bool sets it for the stream — every
    distinct signature of a piece checked once, for streams that relay one update to many stores — and restores
    the previous setting when the generator ends.

    `rlc_group`: 0 leaves the verifier's batch-verification setting (Verifier.set_rlc) alone; 2, 4, ... 64 turns the
    mode on for the stream with that group size and a seed drawn from os.urandom, and restores the previous setting
    (group and seed) when the generator ends."""
    in_flight = int(in_flight)
    if not 1 <= in_flight <= SLOTS:
        raise ValueError(f"in_flight must be 1..{SLOTS}")
    piece_rows = min(MAX_ROWS, int(getattr(verifier, "chunk_rows", MAX_ROWS)))
    gvr = bytes(genesis_validators_root)
    pending = deque()  # (slot or None for an empty item, rows, last piece of its item), oldest first
    parts = []         # the pieces of the oldest item waited for so far
    next_slot = 0
    dedup_before = bool(getattr(verifier, "dedup", False))
    if dedup is not None:
        verifier.set_dedup(bool(dedup))
    rlc_group = int(rlc_group)
    rlc_before = (int(getattr(verifier, "rlc_group", 0)), getattr(verifier, "rlc_seed", None))
    if rlc_group:
        try:
            verifier.set_rlc(rlc_group)
        except Exception:
            if dedup is not None:
                verifier.set_dedup(dedup_before)
            raise

    def finish_oldest():
        slot, rows, last = pending.popleft()
        if slot is not None:
            parts.append(verifier.slot_wait(slot, rows))
        if not last:
            return None
        v = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.uint8)
        r = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.uint8)
        parts.clear()
        return v.astype(bool), r

    try:
        for item in items:
            batch, index = item if isinstance(item, tuple) else (item, None)
            if index is not None:
                index = np.ascontiguousarray(index, np.uint32).reshape(-1)
                if index.shape[0] != batch.n:
                    raise ValueError("store_index needs one entry per update")
            if batch.n == 0:
                pending.append((None, 0, True))
            for lo in range(0, batch.n, piece_rows):
                hi = min(lo + piece_rows, batch.n)
                if sum(1 for p in pending if p[0] is not None) == in_flight:  # the oldest piece holds next_slot
                    while True:
                        waited = pending[0][0] is not None
                        out = finish_oldest()
                        if out is not None:
                            yield out
                        if waited:
                            break
                piece = batch if (lo, hi) == (0, batch.n) else batch.slice(lo, hi)
                if index is None:
                    verifier.validate_async(piece, current_slot, gvr, next_slot)
                else:
                    verifier.validate_stores_async(piece, index[lo:hi], current_slot, gvr, next_slot)
                pending.append((next_slot, hi - lo, hi == batch.n))
                next_slot = (next_slot + 1) % in_flight
        while pending:
            out = finish_oldest()
            if out is not None:
                yield out
    finally:
        for slot, _, _ in pending:  # closed early or failed: nothing stays in flight
            if slot is not None:
                try:
                    verifier.slot_wait(slot, 0)
                except Exception:
                    pass
        if dedup is not None:
            verifier.set_dedup(dedup_before)
        if rlc_group:
            verifier.set_rlc(rlc_before[0], rlc_before[1])


class RelayResult(NamedTuple):
    """relay_updates' result.  `ok[j]`: message j decoded (Verifier.decode_resident's status); `verdict[i]`,
    `reason[i]`: pair i = (message rows[i], store store_index[i]); `dedup`: Verifier.last_dedup of the validation,
    (pairs, distinct BLS items); `batch`: the fanned-out resident table batch, row i = pair i, the caller's to free —
    Verifier.encode_resident(batch, kind, rows=np.flatnonzero(verdict)) serves the accepted pairs on."""
    ok: np.ndarray
    verdict: np.ndarray
    reason: np.ndarray
    dedup: Tuple[int, int]
    batch: ResidentBatch


def relay_updates(verifier: Verifier, messages, kind: str, fork, rows, store_index, current_slot: int,
                  genesis_validators_root: bytes, dedup: bool = True) -> RelayResult:
    """Wire messages in, one verdict per (message, store) pair out, no row on the host: decode_resident, (dedup)
    classify_resident, fan_out(rows, store_index) and validate_resident against the store table that is set, under
    set_dedup(dedup) — each distinct signature checked once — with the verifier's own setting restored afterwards.
    `messages`, `kind`, `fork` as lcv.wire.decode_updates takes them; pair i is message rows[i] for the store of table
    row store_index[i].  A malformed message is an all-zero row (ok False), and its pairs keep that row's verdict and
    reason.  Synchronous; no other call may have slots in flight."""
    ix = np.ascontiguousarray(rows, np.uint32).reshape(-1)
    six = np.ascontiguousarray(store_index, np.uint32).reshape(-1)
    if ix.shape != six.shape:
        raise ValueError("one store_index per row")
    decoded, ok = verifier.decode_resident(messages, kind, fork)
    dedup_before = bool(verifier.dedup)
    try:
        if ix.size and ((ix >= decoded.n).any()):
            raise ValueError(f"rows: message index out of range ({decoded.n} messages)")
        if ix.size == 0:
            return RelayResult(ok, np.zeros(0, bool), np.zeros(0, np.uint8), (0, 0), ResidentBatch(verifier, None, 0, True, decoded.npool))
        if dedup:
            verifier.classify_resident(decoded)
        fanned = verifier.fan_out(decoded, ix, six)
        try:
            verifier.set_dedup(bool(dedup))
            verdict, reason = verifier.validate_resident(fanned, current_slot, genesis_validators_root)
            return RelayResult(ok, verdict.astype(bool), reason, verifier.last_dedup(), fanned)
        except Exception:
            fanned.free()
            raise
    finally:
        decoded.free()
        if verifier.dedup != dedup_before:
            verifier.set_dedup(dedup_before)


class RelayStreamResult(NamedTuple):
    """One item of relay_stream: RelayResult's fields without a resident batch — a relay forwards the bytes it already
    holds — and `fold`: with fold_states, one FoldResult per store row (None for stores without a pair), else None."""
    ok: np.ndarray
    verdict: np.ndarray
    reason: np.ndarray
    dedup: Tuple[int, int]
    fold: Optional[list]


def relay_stream(verifier: Verifier, items: Iterable[tuple], current_slot: int, genesis_validators_root: bytes,
                 in_flight: int = SLOTS, dedup: Optional[bool] = True,
                 fold_states: Optional[Sequence[FoldState]] = None) -> Iterator[RelayStreamResult]:
    """The relay's serving loop: every item (messages, kind, fork, rows, store_index) — as relay_updates takes them,
    kind "finality" or "optimistic", at most 65,536 pairs — goes through Verifier.relay_async on work-space slots
    0 .. in_flight - 1 in turn, and one RelayStreamResult per item is yielded in input order.  The generator waits for
    a slot only when it is about to reuse it (and, after the last item, for what is left).  The store table must be
    set before an item is drawn; no other call may use the verifier's slots while the generator is live; closing it
    early waits for the slots in flight.

    `dedup`: a bool sets Verifier.set_dedup for the stream — each distinct signature of an item checked once — and the
    previous setting is restored when the generator ends, also after an exception; None leaves the setting alone.
    `fold_states`: one FoldState per store row of the table -> every item is folded per store from these states
    (Verifier.validate_stores_fold's results; carrying a store's state from item to item is the caller's)."""
    in_flight = int(in_flight)
    if not 1 <= in_flight <= SLOTS:
        raise ValueError(f"in_flight must be 1..{SLOTS}")
    gvr = bytes(genesis_validators_root)
    pending = deque()  # slots in flight, oldest first
    next_slot = 0
    dedup_before = bool(verifier.dedup)
    if dedup is not None:
        verifier.set_dedup(bool(dedup))

    def finish_oldest():
        slot = pending[0]
        out = verifier.slot_wait_relay(slot)
        pending.popleft()
        return RelayStreamResult(out[0], out[1], out[2], verifier.last_dedup(slot), out[3] if len(out) > 3 else None)

    try:
        for messages, kind, fork, rows, store_index in items:
            if len(pending) == in_flight:  # the oldest item holds next_slot
                yield finish_oldest()
            verifier.relay_async(messages, kind, fork, rows, store_index, current_slot, gvr, next_slot, fold_states)
            pending.append(next_slot)
            next_slot = (next_slot + 1) % in_flight
        while pending:
            yield finish_oldest()
    finally:
        for slot in pending:  # closed early or failed: nothing stays in flight
            try:
                verifier.slot_wait(slot, 0)
            except Exception:
                pass
        if dedup is not None and verifier.dedup != dedup_before:
            verifier.set_dedup(dedup_before)
