"""Shared cases of the resident-classes tests (tests/test_dedup_resident_hostsim.py on the host simulation,
tests/test_dedup_resident_gpu.py on the device): Verifier.classify_resident classes a resident batch where it lies
(F_dedup_key, F_dedup_confirm), Verifier.fan_out gathers a resident batch into a resident table batch, and
lcv.serving.relay_updates strings decode -> classify -> fan-out -> validate_resident together (include/lcv.h "Classes
of a resident batch").

Yardsticks, all exact: the class column of the same rows uploaded under set_dedup(True) (dedup_classes on the host
columns), a dict of the rows' tuple bytes, validation under set_dedup(False), T.take of the downloaded rows.  Rows
are the store-table tests' updates (dedup_cases.base), the reference-serialised messages of tests/golden/wire.npz and
the producer fixture's views; every batch has at most 281 rows.
"""
import ctypes as C

import numpy as np
import pytest

import dedup_cases as D
import producer_batch_cases as PB
import store_serving_cases as SV
import store_table_cases as T
import wire_decode_cases as WD

from lcv import wire
from lcv._native import LcvError, ptr
from lcv.serving import relay_updates

LCV_EINVAL = -1
SIZES = (1, 3, 4, 5, 63, 64, 65, 130)  # the 4-teams-per-wave and the 64-row chunk seams
TUPLE_BYTES = 112 + 64 + 96 + 8


# ------------------------------------------------------------------ plumbing
def tuple_bytes(p):
    """(n, 280) u8: the tuple a class is made of, in the order beacon, bits, signature, signature_slot."""
    slot = np.ascontiguousarray(p.signature_slot, np.uint64).view(np.uint8).reshape(-1, 8)
    return np.concatenate([p.att_beacon, p.sync_bits, p.sync_signature, slot], axis=1)


def first_rows(p):
    """cls[i] = the first row whose tuple equals row i's, from a dict of bytes."""
    seen = {}
    return np.array([seen.setdefault(t.tobytes(), i) for i, t in enumerate(tuple_bytes(p))], np.uint32)


def pattern_rows(v, n):
    """n rows of the three updates in dedup_cases.run_chunks' pattern."""
    _, upd = D.base(v)
    return T.take(upd, (np.arange(n) * 7 + np.arange(n) // 3) % 3)


def classes_both(v, p, hash_bits=64):
    """(host column: upload under set_dedup(True); device column: upload with the mode off, then classify_resident;
    the classes classify_resident counted).  The unclassed batch has no column; classifying twice changes nothing."""
    with D.dedup(v, True, hash_bits):
        rb = v.upload(p)
        try:
            host = v.debug_batch_classes(rb).copy()
        finally:
            rb.free()
    with D.dedup(v, False, hash_bits):
        rb = v.upload(p)
        try:
            with pytest.raises(LcvError, match="no class column"):
                v.debug_batch_classes(rb)
            m = v.classify_resident(rb)
            dev = v.debug_batch_classes(rb).copy()
            assert v.classify_resident(rb) == m and np.array_equal(v.debug_batch_classes(rb), dev)
        finally:
            rb.free()
    return host, dev, m


def check_classes(v, p, hash_bits=64):
    host, dev, m = classes_both(v, p, hash_bits)
    assert np.array_equal(dev, host), np.flatnonzero(dev != host)[:8].tolist()
    assert np.array_equal(host, first_rows(p))
    assert m == len(set(host.tolist()))
    return dev


# ------------------------------------------------------------------ 1: classes equal the host's
def check_sizes(v, n, chunk=None):
    p = pattern_rows(v, n)
    if chunk is None:
        cls = check_classes(v, p)
    else:
        with SV.chunk(v, chunk):
            cls = check_classes(v, p)
    assert len(set(cls.tolist())) == min(n, 3)


def flip_table(v):
    """281 rows: row 0, then row 0 with one bit flipped at each of the 280 tuple byte positions in turn."""
    _, upd = D.base(v)
    p = D.edit(T.take(upd, [0] * (1 + TUPLE_BYTES)), att_beacon=1, sync_bits=1, sync_signature=1, signature_slot=1)
    slot = p.signature_slot.view(np.uint8).reshape(-1, 8)
    for k in range(TUPLE_BYTES):
        col, at = ((p.att_beacon, k) if k < 112 else (p.sync_bits, k - 112) if k < 176 else
                   (p.sync_signature, k - 176) if k < 272 else (slot, k - 272))
        col[1 + k, at] ^= 1 << (k % 8)
    return p


def check_flip_table(v):
    cls = check_classes(v, flip_table(v))
    assert cls.tolist() == list(range(1 + TUPLE_BYTES))


def check_non_tuple_columns(v):
    """Rows that differ in everything but the tuple are one class."""
    _, upd = D.base(v)
    p = D.edit(T.take(upd, [0] * 5), finality_branch=1, nsc_index=1, fin_beacon=1, att_exec=1, nsc_branch=1)
    p.finality_branch[1, 3] ^= 0x20
    p.nsc_index[2] = (int(p.nsc_index[2]) + 1) % p.nsc_pool.shape[0]
    p.fin_beacon[3, 100] ^= 0x01
    p.att_exec[4, 5] ^= 0x80
    p.nsc_branch[4, 17] ^= 0x02
    assert check_classes(v, p).tolist() == [0] * 5


# ------------------------------------------------------------------ 2: collisions
def sixteen_tuples(v):
    """32 rows holding 16 distinct tuples (one signature byte), each twice, in a fixed shuffled order."""
    _, upd = D.base(v)
    order = np.random.default_rng(16).permutation(32) % 16
    p = D.edit(T.take(upd, [0] * 32), sync_signature=1)
    p.sync_signature[:, 50] = order
    return p


def check_collisions(v):
    for p, distinct in ((D.basic_rows(v)[1], 3), (sixteen_tuples(v), 16)):
        runs = [check_classes(v, p, bits) for bits in (64, 1, 0)]
        assert all(np.array_equal(r, runs[0]) for r in runs) and len(set(runs[0].tolist())) == distinct


# ------------------------------------------------------------------ 3: verdicts
def on_off(v, rb, cs, gvr, latency_rows):
    """validate_resident of a classed batch with the mode off and on -> asserts verdicts, reasons, last_dedup and the
    engine; returns the reasons."""
    cls = v.debug_batch_classes(rb)
    distinct = len(set(cls.tolist()))
    with D.latency(v, latency_rows):
        with D.dedup(v, False):
            off = v.validate_resident(rb, cs, gvr)
            assert v.last_dedup() == (rb.n, rb.n)
        with D.dedup(v, True):
            v.engine_log(reset=True)
            on = v.validate_resident(rb, cs, gvr)
            log = v.engine_log(reset=True)
            assert v.last_dedup() == (rb.n, distinct), (v.last_dedup(), distinct)
    assert D.same(off, on), (D.pair(off)[1].tolist(), D.pair(on)[1].tolist())
    if latency_rows:
        assert distinct <= latency_rows
        assert log["fan"] > 0 and log["twin"] > 0 and log["batch"] == 0 and log["lane"] == 0, log
    else:
        assert log["batch"] > 0 and log["lane"] > 0 and log["fan"] == 0 and log["twin"] == 0, log
    return D.pair(on)[1]


def check_verdicts_decoded(v, latency_rows):
    """The golden finality and update messages, three times over, decoded on the device, classed, validated."""
    g = WD.load_updates()
    gvr = g["genesis_validators_root"].tobytes()
    v.set_store(int(g["store_finalized_slot"][0]), g["nsc_pool"][0].tobytes(), g["nsc_pool"][1].tobytes())
    cs = int(g["current_slot"][0])
    for kind in ("finality", "update"):
        msgs, _ = WD.wire_messages(kind)
        rb, ok = wire.decode_updates_device(msgs * 3, kind, verifier=v, classify=True)
        try:
            assert ok.all() and rb.n == 3 * len(msgs)
            cls = v.debug_batch_classes(rb)
            assert np.array_equal(cls, first_rows(v.download(rb))) and len(set(cls.tolist())) <= len(msgs)
            reasons = on_off(v, rb, cs, gvr, latency_rows)
            assert (reasons == 0).any(), kind
        finally:
            rb.free()


def check_verdicts_created(v, latency_rows):
    """A create_updates_resident batch of the producer fixture's views (every case twice), classed, validated."""
    z, cases, views, rows = PB.fixture_views()
    rb, reasons = v.create_updates_resident(views, np.concatenate([rows, rows]))
    try:
        assert reasons.tolist() == [0] * 10
        assert v.classify_resident(rb) <= 5
        assert np.array_equal(v.debug_batch_classes(rb), first_rows(v.download(rb)))
        v.set_store(cases[0]["store_finalized_slot"], z["current_committee"].tobytes(), z["next_committee"].tobytes())
        got = on_off(v, rb, cases[0]["current_slot"], z["genesis_validators_root"].tobytes(), latency_rows)
        assert int(got[0]) == cases[0]["reason"]
    finally:
        rb.free()


# ------------------------------------------------------------------ 4: fan-out rows
FAN_ROWS = [6, 6, 5, 4, 3, 0, 2, 6, 1, 1, 6]  # repeats, a descending run, the last row


def check_fan_out(v):
    p = pattern_rows(v, 7)
    idx = (np.arange(len(FAN_ROWS)) * 5 % 4).astype(np.uint32)
    with D.dedup(v, False):
        rb = v.upload(p)
    made = []
    try:
        src = v.download(rb)
        plain = v.fan_out(rb, FAN_ROWS, idx)  # an unclassed source: an unclassed result
        made.append(plain)
        with pytest.raises(LcvError, match="no class column"):
            v.debug_batch_classes(plain)
        v.classify_resident(rb)
        cls = v.debug_batch_classes(rb)
        for rows, six in ((FAN_ROWS, idx), (None, np.arange(7, dtype=np.uint32) % 4), (FAN_ROWS, None)):
            f = v.fan_out(rb, rows, six)
            made.append(f)
            take = list(range(7)) if rows is None else rows
            assert f.n == len(take) and f.stores == (six is not None) and f.npool == rb.npool
            WD.assert_batches_equal(v.download(f), T.take(src, take), f"fan_out rows={rows is not None} stores={six is not None}")
            assert np.array_equal(v.debug_batch_classes(f), cls[take])
        WD.assert_batches_equal(v.download(plain), T.take(src, FAN_ROWS), "unclassed fan_out")
        WD.assert_batches_equal(v.download(rb), src, "the source is untouched")
    finally:
        for f in made:
            f.free()
        rb.free()


# ------------------------------------------------------------------ 5: the relay
def check_relay(v):
    case, p, index = D.table_case(v, duplicate_row=True)
    cs, gvr = case["current_slot"], case["gvr"]
    with D.dedup(v, False):
        want = D.pair(v.validate_stores(p, index, cs, gvr))
    msgs = wire.encode_updates(T.take(p, [0]), "update", "deneb")
    before = v.dedup
    for dedup, items in ((True, 2), (False, 4)):
        r = relay_updates(v, msgs, "update", "deneb", [0, 0, 0, 0], index, cs, gvr, dedup=dedup)
        try:
            assert r.ok.tolist() == [True] and D.same((r.verdict, r.reason), want), (r.reason.tolist(), want[1].tolist())
            assert r.dedup == (4, items) and r.batch.n == 4 and r.batch.stores and v.dedup == before
            enc = v.encode_resident(r.batch, "update", "deneb", rows=np.flatnonzero(r.verdict))
            assert enc.messages() == [msgs[0]] * int(r.verdict.sum()) and r.verdict.any()
        finally:
            r.batch.free()
    # a malformed message between two good ones: its pairs are the all-zero row's, as decode_resident defines
    three = [msgs[0], msgs[0][:WD.FIXED["update"] - 1], msgs[0]]  # (one byte short of the fixed part)
    rows, stores = [0, 1, 2, 1, 0], np.array([0, 1, 2, 3, 3], np.uint32)
    rb, ok = v.decode_resident(three, "update", "deneb")
    try:
        f = v.fan_out(rb, rows, stores)
        try:
            with D.dedup(v, False):
                want3 = D.pair(v.validate_resident(f, cs, gvr))
        finally:
            f.free()
    finally:
        rb.free()
    r = relay_updates(v, three, "update", "deneb", rows, stores, cs, gvr)
    try:
        assert r.ok.tolist() == ok.tolist() == [True, False, True]
        assert D.same((r.verdict, r.reason), want3) and not r.verdict[[1, 3]].any() and r.verdict[[0, 2]].all()
        assert r.reason[1] == r.reason[3] != 0
        assert r.dedup == (5, 4)  # (good, stores 0 / 2), (good, store 3), (zero row, store 1), (zero row, store 3)
    finally:
        r.batch.free()


# ------------------------------------------------------------------ 6: refusals
def check_refusals(v):
    lib, ctx = v.lib, v.ctx
    case, p, index = D.table_case(v, duplicate_row=True)
    cs, gvr = case["current_slot"], case["gvr"]
    with D.dedup(v, True):
        rb = v.upload(p, index)
        v.validate_resident(rb, cs, gvr)
    made = []
    try:
        assert v.last_dedup() == (4, 2)
        v.engine_log(reset=True)
        m, h = C.c_uint64(77), C.c_void_p(1)
        rows = np.array([0, 1, 4, 9], np.uint32)

        def quiet():
            log = v.engine_log()
            return log["fan"] == log["batch"] == log["twin"] == log["lane"] == 0 and v.last_dedup() == (4, 2)

        for args in ((None, rb.handle, C.byref(m)), (ctx, None, C.byref(m)), (ctx, rb.handle, None)):
            assert lib.lcv_batch_classify(*args) == LCV_EINVAL and quiet()
        assert "null" in lib.lcv_last_error(ctx).decode()
        out = np.zeros(4, np.uint32)
        assert lib.lcv_debug_batch_classes(ctx, None, ptr(out, C.c_uint32)) == LCV_EINVAL
        assert lib.lcv_debug_batch_classes(ctx, rb.handle, None) == LCV_EINVAL
        assert lib.lcv_last_classify_timings(ctx, None) == LCV_EINVAL

        def fan(c=ctx, src=rb.handle, r=ptr(rows, C.c_uint32), s=ptr(index, C.c_uint32), n=4, o=C.byref(h)):
            h.value = 1
            rc = lib.lcv_batch_fan_out(c, src, r, s, n, o)
            assert rc == LCV_EINVAL and quiet() and (o is None or not h.value)  # *out = NULL
            return lib.lcv_last_error(ctx).decode()

        fan(c=None)
        assert "null" in fan(src=None) and "null" in fan(o=None)
        assert "rows[2] = 4" in fan()                       # rows[i] = n_src, the index named
        assert "both null" in fan(r=None, s=None)
        assert "0 < n" in fan(n=0) and "2^32" in fan(n=2 ** 32 - 1)
        assert "must be the source's 4 rows" in fan(r=None, n=3)
        with pytest.raises(LcvError, match=f"status {LCV_EINVAL}"):
            v.fan_out(rb, [], [])
        # a store_index above the table: taken here, refused by the validation, before any launch
        f = v.fan_out(rb, [0, 1], [1, 4])
        made.append(f)
        with pytest.raises(LcvError, match="largest store_index 4"):
            v.validate_resident(f, cs, gvr)
        assert v.engine_log()["fan"] == 0 and v.engine_log()["batch"] == 0
        # classify under a multi-stream pipeline succeeds; the mode itself is refused, as ever
        with SV.pipeline(v, 2, 2):
            assert v.classify_resident(rb) == 1
            with pytest.raises(LcvError, match=f"status {LCV_EINVAL}"):
                v.set_dedup(True)
            assert v.dedup is False
            assert D.same(v.validate_resident(rb, cs, gvr), D.pair(v.validate_stores(p, index, cs, gvr)))
            assert v.last_dedup() == (4, 4)
    finally:
        for f in made:
            f.free()
        rb.free()
    assert v.classify_resident(v.decode_resident([], "update")[0]) == 0  # no rows: 0 classes


# ------------------------------------------------------------------ 7: existing behaviour
def check_existing_behaviour(v):
    g = WD.load_updates()
    gvr = g["genesis_validators_root"].tobytes()
    v.set_store(int(g["store_finalized_slot"][0]), g["nsc_pool"][0].tobytes(), g["nsc_pool"][1].tobytes())
    cs = int(g["current_slot"][0])
    msgs, _ = WD.wire_messages("finality")
    assert v.lib.lcv_stage_name(22) == b"wire_encode" and v.lib.lcv_stage_name(23) == b"?"
    rb, ok = v.decode_resident(msgs * 2, "finality")
    try:
        with D.dedup(v, True):  # never classified: every row runs
            never = v.validate_resident(rb, cs, gvr)
            assert v.last_dedup() == (rb.n, rb.n)
        assert sum(v.last_timings().values()) > 0
        m = v.classify_resident(rb)
        t = v.last_timings()
        assert len(t) == 23 and all(x == 0.0 for x in t.values()), t
        keys, confirms = v.last_classify_timings()
        assert keys > 0 and confirms > 0 and m <= len(msgs)
        with D.dedup(v, True):
            assert D.same(v.validate_resident(rb, cs, gvr), D.pair(never)) and v.last_dedup() == (rb.n, m)
    finally:
        rb.free()
