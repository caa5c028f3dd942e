"""Shared cases of the deduplication tests (tests/test_dedup_hostsim.py on the host simulation, tests/test_dedup_gpu.py
on the device): with Verifier.set_dedup(True) the BLS half of validation runs once per distinct BLS item of a chunk
— (attested beacon header, signature_slot, sync bits, signature, committee row the signature is checked against) —
and every row takes its verdict from its item (include/lcv.h "Deduplicated signatures").

The yardstick of every case is the same call under set_dedup(False): verdict and reason bytes must be equal, and
Verifier.last_dedup must report the rows and the distinct items the case was built with.  Where the reasons are
known from the reference (sync-protocol.md:386-465, or the reference-exec'd golden fixture) they are asserted too.
Exact equality everywhere, no tolerance.  Rows are built from the store-table tests' updates (store_table_cases:
A and B signed by committee c0 in the store's period, C signed by c1 in the next one), so nothing new is signed.
"""
import contextlib

import numpy as np

import golden_cases as G
import store_table_cases as T

LCV_EINVAL = -1
UNKNOWN = T.UNKNOWN
SLOTS_PER_PERIOD = 32 * 256  # mainnet


# ------------------------------------------------------------------ plumbing
@contextlib.contextmanager
def dedup(v, on=True, hash_bits=64):
    """set_dedup(on) for the block; the verifier is shared by the session, so off again afterwards."""
    v.debug_dedup_hash_bits(hash_bits)
    v.set_dedup(on)
    try:
        yield
    finally:
        v.set_dedup(False)
        v.debug_dedup_hash_bits(64)


@contextlib.contextmanager
def latency(v, rows):
    prev = v.latency_mode
    v.set_latency_mode(rows)
    try:
        yield
    finally:
        v.set_latency_mode(prev)


def pair(res):
    """(verdicts as bool, reasons) of any validate result."""
    return np.asarray(res[0]).astype(bool), np.asarray(res[1], np.uint8)


def same(a, b):
    a, b = pair(a), pair(b)
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def off_on(v, call, slot=0, hash_bits=64):
    """call() with the mode off, then on -> (result off, result on, last_dedup(slot) off, last_dedup(slot) on)."""
    with dedup(v, False):
        off = call()
        d_off = v.last_dedup(slot)
    with dedup(v, True, hash_bits):
        on = call()
        d_on = v.last_dedup(slot)
    return off, on, d_off, d_on


def check(v, call, rows, items, slot=0, hash_bits=64):
    """The yardstick of every case: the call's verdicts and reasons with the mode on equal those with it off, rows ==
    items with it off, and (rows, items) as built with it on.  Returns the reasons."""
    off, on, d_off, d_on = off_on(v, call, slot, hash_bits)
    assert same(off, on), (pair(off)[1].tolist(), pair(on)[1].tolist())
    ok, reason = pair(on)
    assert np.array_equal(ok, reason == 0)
    assert d_off == (rows, rows), d_off
    assert d_on == (rows, items), d_on
    return reason.tolist()


def base(v):
    """(semantics case of the store-table tests, its updates A, B, C) with the single store (fin, c0, c1) set, under
    which all three are valid."""
    case = T.semantics_case(v)
    c = T.committees(v)
    v.set_store(case["stores"][0][0], c[0].ssz, c[1].ssz)
    return case, case["updates"]


def edit(p, **cols):
    """A copy of p with the given columns replaced by writable copies (rows are edited in place afterwards)."""
    from lcv.device import PackedUpdates
    from dataclasses import fields
    kw = {f.name: getattr(p, f.name) for f in fields(p)}
    for k in cols:
        kw[k] = np.array(kw[k], copy=True)
    return PackedUpdates(**kw)


# ------------------------------------------------------------------ 1: basic merge
def basic_rows(v):
    """Six rows against one store: 0, 2, 5 one valid update, 1, 3 another, 4 = row 0 with one signature byte flipped."""
    case, upd = base(v)
    p = edit(T.take(upd, [0, 1, 0, 1, 0, 0]), sync_signature=1)
    p.sync_signature[4, 40] ^= 0x04
    return case, p


BASIC_REASONS = [0, 0, 0, 0, 14, 0]  # row 4: LCV_R_SIGNATURE (:464)


def run_basic(v, latency_rows, hash_bits=64):
    """Case 1 on one engine -> (reasons, engine log of the deduplicated call)."""
    case, p = basic_rows(v)
    with latency(v, latency_rows):
        reasons = check(v, lambda: v.validate(p, case["current_slot"], case["gvr"]), 6, 3, hash_bits=hash_bits)
        with dedup(v, True, hash_bits):
            v.engine_log(reset=True)
            v.validate(p, case["current_slot"], case["gvr"])
            log = v.engine_log(reset=True)
    return reasons, log


# ------------------------------------------------------------------ 2: shared item, different pre-checks
def run_shared_item(v):
    """A valid; B = A with a corrupted finality branch (reason 10, same item); C = A with no participation bits
    (reason 1, another tuple) -> reasons; 2 items."""
    case, upd = base(v)
    p = edit(T.take(upd, [0, 0, 0]), finality_branch=1, sync_bits=1)
    p.finality_branch[1, 7] ^= 0x10
    p.sync_bits[2, :] = 0
    return check(v, lambda: v.validate(p, case["current_slot"], case["gvr"]), 3, 2)


# ------------------------------------------------------------------ 3: shared failing item
def run_shared_failure(v, signature):
    """Four copies of update A carrying `signature` (96 bytes) instead of its own -> reasons; 1 item."""
    case, upd = base(v)
    p = edit(T.take(upd, [0, 0, 0, 0]), sync_signature=1)
    p.sync_signature[:] = np.frombuffer(bytes(signature), np.uint8)
    return check(v, lambda: v.validate(p, case["current_slot"], case["gvr"]), 4, 1)


def wrong_key_signature(v):
    """A valid G2 point that is no signature of update A: update B's."""
    _, upd = base(v)
    assert not np.array_equal(upd.att_beacon[0], upd.att_beacon[1])
    return upd.sync_signature[1].tobytes()


def non_subgroup_signature():
    """A curve point outside G2 (tests/g2_edge_points.py): the fused subgroup check rejects it."""
    from oracle import bls12_381 as B
    return B.g2_compress(B.g2_add(B.g2_mul(B.G2_GEN, 0x1234567), B.g2_point_of_order(13)))


# ------------------------------------------------------------------ 4: store table
def table_case(v, duplicate_row):
    """Update A to four stores: 0 and 1 hold the same current (c0) and next (c1) rows, 2 the same current and an
    unknown next, 3 is finalized one period earlier, so A's signature falls into ITS next period and is checked
    against its next row: c1 (the signature fails), or — duplicate_row — a second committee row with c0's content
    (the signature holds, and the row still is another item: rows of equal content are not merged)."""
    case, upd = base(v)
    c = T.committees(v)
    fin = case["stores"][0][0]
    rows = [c[0].ssz, c[1].ssz, c[2].ssz] + ([c[0].ssz] if duplicate_row else [])
    stores = [(fin, 0, 1), (fin, 0, 1), (fin, 0, UNKNOWN), (fin - SLOTS_PER_PERIOD, 2, 3 if duplicate_row else 1)]
    v.set_store_table(np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), T.SC_BYTES), [s[0] for s in stores],
                      [s[1] for s in stores], [s[2] for s in stores])
    return case, T.take(upd, [0, 0, 0, 0]), np.arange(4, dtype=np.uint32)


def run_table(v, duplicate_row, hash_bits=64):
    """-> reasons of the four rows; stores 0, 1, 2 share an item, store 3 has its own."""
    case, p, index = table_case(v, duplicate_row)
    return check(v, lambda: v.validate_stores(p, index, case["current_slot"], case["gvr"]), 4, 2, hash_bits=hash_bits)


# ------------------------------------------------------------------ 5: golden replay
def run_golden(v):
    """Every case of lc_updates.npz three times, shuffled by a fixed permutation, through the store table (a store
    row per (finalized slot, next known) of the fixture, one call per current_slot) with the mode on -> (reasons in
    shuffled order, the fixture's reference-exec'd reasons in that order, items summed over the calls, cases)."""
    from lcv.device import PackedUpdates
    g = G.load_updates()
    n = len(g["expected_reason"])
    gvr = g["genesis_validators_root"].tobytes()
    stores = sorted({(int(g["store_finalized_slot"][i]), int(g["store_next_known"][i])) for i in range(n)})
    v.set_store_table(g["nsc_pool"][:2], [s[0] for s in stores], [0] * len(stores), [1 if s[1] else UNKNOWN for s in stores])
    p = PackedUpdates(nsc_pool=g["nsc_pool"], nsc_index=g["nsc_index"], signature_slot=g["signature_slot"],
                      **{k: g[k] for k in G.COLS})
    index = np.array([stores.index((int(g["store_finalized_slot"][i]), int(g["store_next_known"][i]))) for i in range(n)], np.uint32)
    case_of = np.tile(np.arange(n), 3)[np.random.default_rng(2024).permutation(3 * n)]
    got = np.full(3 * n, 255, np.uint8)
    items = 0
    with dedup(v, True):
        for cs in sorted({int(s) for s in g["current_slot"]}):
            rows = [j for j in range(3 * n) if int(g["current_slot"][case_of[j]]) == cs]
            ok, reason = v.validate_stores(T.take(p, case_of[rows]), index[case_of[rows]], cs, gvr)
            assert np.array_equal(ok, reason == 0)
            got[rows] = reason
            d = v.last_dedup()
            assert d[0] == len(rows) and d[1] <= len(set(case_of[rows].tolist())), (cs, d)
            items += d[1]
    return got, g["expected_reason"][case_of], items, n


# ------------------------------------------------------------------ 7: engine by items
def run_engine_by_items(v):
    """70 rows made of 2 distinct updates under latency mode 64, with the mode on only -> (reasons of the 70 rows,
    the 2-row call's reasons expanded, engine log of the 70-row call, last_dedup)."""
    case, upd = base(v)
    pattern = np.arange(70) % 2
    with latency(v, 64), dedup(v, True):
        two = pair(v.validate(T.take(upd, [0, 1]), case["current_slot"], case["gvr"]))
        v.engine_log(reset=True)
        got = pair(v.validate(T.take(upd, pattern), case["current_slot"], case["gvr"]))
        log = v.engine_log(reset=True)
        d = v.last_dedup()
    assert np.array_equal(got[0], got[1] == 0)
    return got[1], two[1][pattern], log, d


# ------------------------------------------------------------------ 8: chunks
def run_chunks(v):
    """130 rows made of the 3 distinct updates under 64-row chunks (64 + 64 + 2, rotating over the slots) -> (reasons,
    last_dedup on, the sum over the chunks of their distinct updates)."""
    import store_serving_cases as SV
    case, upd = base(v)
    pattern = (np.arange(130) * 7 + np.arange(130) // 3) % 3
    per_chunk = sum(len(set(pattern[b:b + 64].tolist())) for b in range(0, 130, 64))
    p = T.take(upd, pattern)
    with SV.chunk(v, 64):
        off, on, d_off, d_on = off_on(v, lambda: v.validate(p, case["current_slot"], case["gvr"]))
    assert same(off, on) and d_off == (130, 130)
    assert np.array_equal(pair(on)[0], pair(on)[1] == 0)
    return pair(on)[1], d_on, per_chunk


# ------------------------------------------------------------------ 9: other shapes
def run_async(v):
    """A deduplicated table batch on slot 2 and a single-store batch on slot 5 in flight at once -> asserts inside."""
    case, p, index = table_case(v, True)
    _, q = basic_rows(v)
    cs, gvr = case["current_slot"], case["gvr"]

    def both():
        v.validate_stores_async(p, index, cs, gvr, 2)
        v.validate_async(q, cs, gvr, 5)
        return v.slot_wait(2, p.n), v.slot_wait(5, q.n), v.last_dedup(2), v.last_dedup(5)

    with dedup(v, False):
        off = both()
    with dedup(v, True):
        on = both()
    assert same(off[0], on[0]) and same(off[1], on[1])
    assert pair(on[1])[1].tolist() == BASIC_REASONS
    assert off[2:] == ((4, 4), (6, 6)) and on[2:] == ((4, 2), (6, 3)), (off[2:], on[2:])


def run_resident(v):
    """upload(..., store_index) with the mode on, then validate_resident and validate_resident_async; a batch uploaded
    with the mode off and validated with it on reports items == rows -> asserts inside."""
    case, p, index = table_case(v, True)
    cs, gvr = case["current_slot"], case["gvr"]
    with dedup(v, False):
        want = pair(v.validate_stores(p, index, cs, gvr))
        plain = v.upload(p, index)
    try:
        with dedup(v, True):
            rb = v.upload(p, index)
            try:
                assert same(v.validate_resident(rb, cs, gvr), want) and v.last_dedup() == (4, 2)
                v.validate_resident_async(rb, cs, gvr, 3)
                assert same(v.slot_wait(3, p.n), want) and v.last_dedup(3) == (4, 2)
                assert same(v.validate_resident(plain, cs, gvr), want) and v.last_dedup() == (4, 4)
            finally:
                rb.free()
        # with the mode off a batch that has its class column is validated row by row
        with dedup(v, True):
            rb = v.upload(p, index)
        try:
            assert same(v.validate_resident(rb, cs, gvr), want) and v.last_dedup() == (4, 4)
        finally:
            rb.free()
    finally:
        plain.free()
    # a single-store resident batch
    case, q = basic_rows(v)
    with dedup(v, True):
        rq = v.upload(q)
        try:
            got = v.validate_resident(rq, cs, gvr)
            assert pair(got)[1].tolist() == BASIC_REASONS and v.last_dedup() == (6, 3)
        finally:
            rq.free()


def run_fold(v):
    """validate_fold and validate_stores_fold with the mode on and off -> asserts inside (results field by field)."""
    from dataclasses import asdict
    from lcv.device import FoldState
    case, q = basic_rows(v)
    cs, gvr = case["current_slot"], case["gvr"]
    off, on, d_off, d_on = off_on(v, lambda: v.validate_fold(q, cs, gvr, FoldState()))
    assert same(off, on) and asdict(off[2]) == asdict(on[2]) and (d_off, d_on) == ((6, 6), (6, 3))
    assert pair(on)[1].tolist() == BASIC_REASONS
    case, p, index = table_case(v, True)
    states = [FoldState() for _ in range(4)]
    off, on, d_off, d_on = off_on(v, lambda: v.validate_stores_fold(p, index, cs, gvr, states))
    assert same(off, on) and (d_off, d_on) == ((4, 4), (4, 2))
    assert [asdict(r) for r in off[2]] == [asdict(r) for r in on[2]] and all(r is not None for r in on[2])


def run_stream(v):
    """validate_stream(dedup=True) over single-store and table items; the verifier's setting is restored."""
    from lcv.serving import validate_stream
    case, p, index = table_case(v, True)
    _, q = basic_rows(v)
    cs, gvr = case["current_slot"], case["gvr"]
    items = [(p, index), q, (T.take(p, []), index[:0]), q, (p, index)]
    with dedup(v, False):
        want = list(validate_stream(v, iter(items), cs, gvr, in_flight=2))
        got = list(validate_stream(v, iter(items), cs, gvr, in_flight=2, dedup=True))
        assert v.dedup is False
    assert len(got) == len(want) == 5 and all(same(a, b) for a, b in zip(got, want))
    assert got[1][1].tolist() == BASIC_REASONS
    with dedup(v, True):
        assert same(list(validate_stream(v, iter([q]), cs, gvr, dedup=None))[0], want[1]) and v.dedup is True
        list(validate_stream(v, iter([q]), cs, gvr, dedup=False))
        assert v.dedup is True


def run_pipeline_refused(v):
    """set_dedup(True) with a multi-stream pipeline: LCV_EINVAL from whichever call comes second."""
    from lcv._native import LcvError
    import pytest
    try:
        v.set_dedup(True)
        with pytest.raises(LcvError, match=f"status {LCV_EINVAL}"):
            v.set_pipeline(2, 2)
        assert v.pipeline == (1, 1)
        v.set_pipeline(1, 4)  # one stream: no slicing
        v.set_pipeline(1, 1)
        v.set_dedup(False)
        v.set_pipeline(2, 2)
        with pytest.raises(LcvError, match=f"status {LCV_EINVAL}"):
            v.set_dedup(True)
        assert v.dedup is False
    finally:
        v.set_dedup(False)
        v.set_pipeline(1, 1)


# ------------------------------------------------------------------ 10: mode off
def run_mode_off(v, fresh):
    """`fresh`: a context of v's backend on which the mode was never on.  The engine log of a 6-row call there, and
    of the same call after the mode was turned on and off again -> (before, after)."""
    case, p = basic_rows(v)
    c = T.committees(v)
    fresh.set_store(case["stores"][0][0], c[0].ssz, c[1].ssz)
    call = lambda: fresh.validate(p, case["current_slot"], case["gvr"])  # noqa: E731
    fresh.engine_log(reset=True)
    want = pair(call())
    before = fresh.engine_log(reset=True)
    with dedup(fresh, True):
        assert same(call(), want) and fresh.last_dedup() == (6, 3)
    fresh.engine_log(reset=True)
    assert same(call(), want) and fresh.last_dedup() == (6, 6)
    return before, fresh.engine_log(reset=True)
