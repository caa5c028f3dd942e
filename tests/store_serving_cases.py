"""Shared cases of the store-table serving tests (tests/test_store_serving_hostsim.py on the host simulation,
tests/test_store_serving_gpu.py on the device): table batches — update i against store row store_index[i] — in the
resident, asynchronous, piped and sharded shapes, and lcv.serving.validate_stream over them.

The yardstick is always the synchronous validate_stores (lcv_validate_updates_stores) on the same rows and the same
table, which tests/store_table_cases.py pins to the single-store path and the goldens; where the rows are the
10-row semantics batch, store_table_cases.SEM_EXPECTED is a second one.  Everything is exact equality.
"""
import contextlib
import os

import numpy as np

import store_table_cases as T

LCV_EINVAL, LCV_ESTATE = -1, -4


# ------------------------------------------------------------------ inputs
def sem_batch(v):
    """(case, the 10-row semantics batch, its store_index)."""
    case = T.semantics_case(v)
    return case, T.take(case["updates"], [u for u, _ in case["rows"]]), np.array([s for _, s in case["rows"]], np.uint32)


def tiled(v, n):
    """n rows: tiles of the semantics batch's 10 (update, store) rows, odd tiles with the stores rotated by 5 rows
    (store_table_cases.run_chunks' rows), so that store rows change inside and across chunks of 64 and all six
    stores occur.  Repeated rows cost no signing."""
    case = T.semantics_case(v)
    rows = [(case["rows"][i % 10][0], case["rows"][(i % 10 + 5 * ((i // 10) % 2)) % 10][1]) for i in range(n)]
    return case, T.take(case["updates"], [u for u, _ in rows]), np.array([s for _, s in rows], np.uint32)


def sync(v, case, p, index):
    """The yardstick: (verdicts as bool, reasons) of the synchronous call under the table that is set."""
    ok, reason = v.validate_stores(p, index, case["current_slot"], case["gvr"])
    assert np.array_equal(ok, reason == 0)
    return ok, reason


def same(got, want):
    """(verdict bytes or bools, reasons) == the yardstick's."""
    return np.array_equal(np.asarray(got[0]).astype(bool), want[0]) and np.array_equal(got[1], want[1])


@contextlib.contextmanager
def chunk(v, rows):
    prev = v.chunk_rows
    v.debug_set_chunk(rows)
    try:
        yield
    finally:
        v.debug_set_chunk(prev)


@contextlib.contextmanager
def pipeline(v, streams, chunks):
    prev = v.pipeline
    v.set_pipeline(streams, chunks)
    try:
        yield
    finally:
        v.set_pipeline(*prev)


def is_hostsim(v):
    return "hostsim" in os.path.basename(v.lib.path)


def device_bytes(v, n):
    """A buffer of n bytes the backend's kernels can write: (its address, a function that returns its content as a
    numpy array and frees it).  On the host simulation device memory is host memory; on the device the buffer comes
    from the HIP runtime liblcv.so is linked against, which the process has already loaded."""
    if is_hostsim(v):
        a = np.full(n, 255, np.uint8)
        return a.ctypes.data, lambda: a.copy()
    import ctypes as C
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d = C.c_void_p()
    assert hip.hipSetDevice(v.device) == 0 and hip.hipMalloc(C.byref(d), n) == 0
    assert hip.hipMemset(d, 255, n) == 0 and hip.hipDeviceSynchronize() == 0

    def read():
        out = np.zeros(n, np.uint8)
        rc = hip.hipMemcpy(out.ctypes.data, d, n, 2)  # hipMemcpyDeviceToHost
        hip.hipFree(d)
        assert rc == 0
        return out

    return d.value, read


# ------------------------------------------------------------------ 1: resident
def run_resident(v):
    """The 10-row semantics batch uploaded with its index -> (reasons of validate_resident, verdict bytes of
    validate_resident_dev copied back, the synchronous yardstick)."""
    case, p, index = sem_batch(v)
    T.set_table(v, case)
    want = sync(v, case, p, index)
    rb = v.upload(p, index)
    try:
        assert rb.stores and not v.upload(p).stores
        got = v.validate_resident(rb, case["current_slot"], case["gvr"])
        addr, read = device_bytes(v, p.n)
        v.validate_resident_dev(rb, case["current_slot"], case["gvr"], addr)
        dev = read()
    finally:
        rb.free()
    return got, dev, want


# ------------------------------------------------------------------ 2: chunks
def run_chunks(v):
    """130 rows under 64-row chunks (64 + 64 + 2, rotating over the slots) through the resident path, and the same
    rows through validate_stores_async in one piece -> (resident, async, yardstick under 64-row chunks, yardstick
    in one chunk)."""
    case, p, index = tiled(v, 130)
    assert any(index[i] != index[i + 64] for i in range(64)) and len(set(index[:64].tolist())) > 1
    T.set_table(v, case)
    want1 = sync(v, case, p, index)
    rb = v.upload(p, index)
    try:
        with chunk(v, 64):
            want64 = sync(v, case, p, index)
            res = v.validate_resident(rb, case["current_slot"], case["gvr"])
    finally:
        rb.free()
    v.validate_stores_async(p, index, case["current_slot"], case["gvr"], 3)
    return res, v.slot_wait(3, p.n), want64, want1


# ------------------------------------------------------------------ 3: slots
def run_slots(v):
    """Table batches in flight: two resident ones on slots 0 and 1, host-input ones on all eight slots, and a
    single-store batch beside a table batch.  Asserts inside; returns the event pool before and after."""
    case, p, index = sem_batch(v)
    q, qindex = T.take(p, list(range(9, -1, -1))), np.roll(index[::-1], 3).astype(np.uint32)  # a different batch
    cs, gvr = case["current_slot"], case["gvr"]
    T.set_table(v, case)
    v.set_store(*T.store_key(case, 1))
    want_p, want_q = sync(v, case, p, index), sync(v, case, q, qindex)
    assert list(want_p[1]) == T.SEM_EXPECTED and list(want_q[1]) != list(want_p[1])
    single = v.validate(p, cs, gvr)  # every row under store 1 alone
    assert list(single[1]) != list(want_p[1])
    rp, rq, rs = v.upload(p, index), v.upload(q, qindex), v.upload(p)
    pool0 = v.event_pool()
    try:
        for _ in range(3):
            v.validate_resident_async(rp, cs, gvr, 0)
            v.validate_resident_async(rq, cs, gvr, 1)
            assert same(v.slot_wait(0, p.n), want_p)
            assert same(v.slot_wait(1, q.n), want_q)
        for rep in range(3):
            for s in range(8):
                x = (p, index) if (s + rep) % 2 == 0 else (q, qindex)
                v.validate_stores_async(x[0], x[1], cs, gvr, s)
            for s in range(8):
                assert same(v.slot_wait(s, 10), want_p if (s + rep) % 2 == 0 else want_q), (rep, s)
        # the store of set_store and the store table are independent, also in flight side by side
        v.validate_resident_async(rs, cs, gvr, 0)
        v.validate_resident_async(rp, cs, gvr, 1)
        assert same(v.slot_wait(0, p.n), single)
        assert same(v.slot_wait(1, p.n), want_p)
        v.validate_stores_async(q, qindex, cs, gvr, 0)
        v.validate_async(p, cs, gvr, 1)
        assert same(v.slot_wait(0, q.n), want_q)
        assert same(v.slot_wait(1, p.n), single)
    finally:
        for r in (rp, rq, rs):
            r.free()
    return pool0, v.event_pool()


# ------------------------------------------------------------------ 4: pipeline
def run_pipeline(v):
    """256 rows (128 x 2 slices: the smallest batch the slicing accepts) over the six stores, serial shape and
    set_pipeline(2, 2) -> ((sync, resident) serial, (sync, resident) piped)."""
    case, p, index = tiled(v, 256)
    assert set(index.tolist()) == set(range(6))
    T.set_table(v, case)
    rb = v.upload(p, index)
    out = []
    try:
        for shape in ((1, 1), (2, 2)):
            with pipeline(v, *shape):
                out.append((sync(v, case, p, index), v.validate_resident(rb, case["current_slot"], case["gvr"])))
    finally:
        rb.free()
    return out


# ------------------------------------------------------------------ 5: table replaced
def run_table_replaced(v, tiles=1):
    """A batch in flight on slot 1 when set_store_table brings a table with other verdicts (the stores in reverse
    order) -> (slot 1's result, the same resident batch validated again, yardstick under the old table, yardstick
    under the new one)."""
    case, p, index = sem_batch(v)
    if tiles > 1:
        p, index = T.take(p, list(range(10)) * tiles), np.tile(index, tiles)
    cs, gvr = case["current_slot"], case["gvr"]
    new = dict(case, stores=case["stores"][::-1])
    T.set_table(v, new)
    want_new = sync(v, case, p, index)
    T.set_table(v, case)
    want_old = sync(v, case, p, index)
    assert list(want_old[1][:10]) == T.SEM_EXPECTED and list(want_new[1]) != list(want_old[1])
    rb = v.upload(p, index)
    try:
        v.validate_resident_async(rb, cs, gvr, 1)
        T.set_table(v, new)
        first = v.slot_wait(1, p.n)
        again = v.validate_resident(rb, cs, gvr)
    finally:
        rb.free()
    return first, again, want_old, want_new


# ------------------------------------------------------------------ 6: host checks, no launch
def run_host_checks(v, fresh):
    """Argument errors caught on the host before any kernel; `fresh` is a verifier of the same backend on which no
    table has been set.  Asserts inside; returns the reasons of a correct call after each refused one."""
    from lcv._native import LcvError
    case, p, index = sem_batch(v)
    cs, gvr = case["current_slot"], case["gvr"]
    after = []

    def refused(call, *words):
        log = v.engine_log()
        try:
            call()
        except LcvError as e:
            msg = str(e)
        else:
            raise AssertionError("the call was accepted")
        assert all(w in msg for w in words), msg
        assert v.engine_log() == log  # nothing was launched
        T.set_table(v, case)
        after.append(list(sync(v, case, p, index)[1]))

    rb = v.upload(p, index)  # largest index 5
    try:
        T.set_table(v, dict(case, stores=case["stores"][:3]))
        refused(lambda: v.validate_resident(rb, cs, gvr), f"status {LCV_EINVAL}", "5", "nstore 3")
        T.set_table(v, dict(case, stores=case["stores"][:3]))
        refused(lambda: v.validate_resident_async(rb, cs, gvr, 1), f"status {LCV_EINVAL}", "5", "nstore 3")
        bad = index.copy()
        bad[7] = 6
        refused(lambda: v.validate_stores_async(p, bad, cs, gvr, 0), f"status {LCV_EINVAL}", "store_index[7] = 6", "nstore 6")
        refused(lambda: v.validate_stores_async(p, index, cs, gvr, 8), f"status {LCV_EINVAL}", "slot")
        after.append(list(v.validate_resident(rb, cs, gvr)[1]))
    finally:
        rb.free()
    # no table set: LCV_ESTATE from every entry, resident and host-input
    rf = fresh.upload(p, index)  # (an upload needs no table)
    try:
        for call in (lambda: fresh.validate_resident(rf, cs, gvr), lambda: fresh.validate_resident_async(rf, cs, gvr, 0),
                     lambda: fresh.validate_stores_async(p, index, cs, gvr, 0)):
            try:
                call()
            except LcvError as e:
                assert f"status {LCV_ESTATE}" in str(e) and "lcv_set_store_table" in str(e), str(e)
            else:
                raise AssertionError("validated without a table")
        T.set_table(fresh, case)
        after.append(list(fresh.validate_resident(rf, cs, gvr)[1]))
    finally:
        rf.free()
    return after


# ------------------------------------------------------------------ 7: sharded
def run_sharded(v, key):
    """multi.validate_sharded(..., store_index=...) on one rank, and the per-slot all-gather behind a table batch
    -> (sharded verdicts, slot all-gather verdicts, yardstick)."""
    from lcv import multi
    case, p, index = sem_batch(v)
    cs, gvr = case["current_slot"], case["gvr"]
    T.set_table(v, case)
    want = sync(v, case, p, index)
    comm = multi.Comm(v, 1, 0, key=key)
    try:
        full = multi.validate_sharded(v, p, cs, gvr, comm, store_index=index)
        rb = v.upload(p, index)
        try:
            v.validate_resident_async(rb, cs, gvr, 2)
            g = comm.slot_allgather(2, p.n, 16)
        finally:
            rb.free()
        assert not g[p.n:].any()
    finally:
        comm.close()
    return full, g[:p.n].astype(bool), want


# ------------------------------------------------------------------ 8: validate_stream
def run_stream(v, in_flight):
    """Single-store and table items mixed, one of 130 rows under 64-row chunks (cut into 64 + 64 + 2), an empty one
    -> (results in input order, the synchronous yardsticks)."""
    from lcv.serving import validate_stream
    case, p, index = sem_batch(v)
    _, big, big_index = tiled(v, 130)
    cs, gvr = case["current_slot"], case["gvr"]
    T.set_table(v, case)
    v.set_store(*T.store_key(case, 1))
    q, qindex = T.take(p, [3, 1, 8]), index[[5, 0, 2]]
    items = [(p, index), p, (big, big_index), q, (q, qindex), (T.take(p, []), index[:0]), big, (p, index), p, (q, qindex)]
    want = [sync(v, case, *it) if isinstance(it, tuple) and it[0].n else
            (np.zeros(0, bool), np.zeros(0, np.uint8)) if isinstance(it, tuple) else v.validate(it, cs, gvr) for it in items]
    with chunk(v, 64):
        got = list(validate_stream(v, iter(items), cs, gvr, in_flight=in_flight))
    return got, want
