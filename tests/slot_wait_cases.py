"""Shared cases of the slot-wait tests (tests/test_slot_wait_hostsim.py on the host simulation,
tests/test_slot_wait_gpu.py on the device): what each of the four waits (include/lcv.h: lcv_slot_wait,
lcv_slot_wait_fold, lcv_slot_wait_stores_fold, lcv_slot_wait_relay without and with fold_out) returns for each of the
seven ways a batch is put on a work-space slot, cell by cell.

    slot's last batch            slot_wait  _fold    _stores_fold  _relay   _relay + fold_out
    validate_resident_async      OK         ESTATE   ESTATE        ESTATE   ESTATE
    validate_async               OK         ESTATE   ESTATE        ESTATE   ESTATE
    validate_stores_async        OK         ESTATE   ESTATE        ESTATE   ESTATE
    validate_async_fold          OK         OK       ESTATE        ESTATE   ESTATE
    validate_stores_async_fold   OK         ESTATE   OK            ESTATE   ESTATE
    relay_async without fold_in  OK         ESTATE   ESTATE        OK       ESTATE
    relay_async with fold_in     OK         ESTATE   ESTATE        OK       OK

An OK cell hands out exactly what the synchronous entry gives for the same rows (lcv_validate_updates,
lcv_validate_updates_stores, lcv_validate_fold, lcv_validate_stores_fold; for the relay the synchronous relay of
lcv.serving.relay_updates and lcv_validate_stores_fold on the host-decoded pairs), and hands it out again when the wait
is repeated: a wait does not consume.  Everything is bytes: equality, no tolerance.

Fixture: the two-store table and the first 12 rows of the golden sequence that store_fold_multi_cases.check_async
uses; three reference-serialised finality messages of tests/golden/wire.npz for the relay, six pairs.  The synchronous
results are computed once and shared."""
import ctypes as C

import numpy as np

import store_cases
import store_fold_cases as SF
import store_fold_multi_cases as SM
import wire_decode_cases as WD

from lcv import runtime, wire
from lcv._native import FoldResultC, ptr
from lcv.device import FoldState
from lcv.serving import relay_updates

OK, EINVAL, ESTATE = 0, -1, -4
WAITS = ("slot_wait", "slot_wait_fold", "slot_wait_stores_fold", "slot_wait_relay", "slot_wait_relay+fold_out")
TABLE = {
    "validate_resident_async": (OK, ESTATE, ESTATE, ESTATE, ESTATE),
    "validate_async": (OK, ESTATE, ESTATE, ESTATE, ESTATE),
    "validate_stores_async": (OK, ESTATE, ESTATE, ESTATE, ESTATE),
    "validate_async_fold": (OK, OK, ESTATE, ESTATE, ESTATE),
    "validate_stores_async_fold": (OK, ESTATE, OK, ESTATE, ESTATE),
    "relay_async": (OK, ESTATE, ESTATE, OK, ESTATE),
    "relay_async+fold_in": (OK, ESTATE, ESTATE, OK, OK),
}
ENTRIES = tuple(TABLE)
SLOT = 5
NSTORE = 2
PAIR_ROWS = np.array([0, 1, 2, 1, 0, 2], np.uint32)
PAIR_STORES = np.array([0, 1, 0, 0, 1, 1], np.uint32)
SENTINEL = 0xEE

_cache = {}


def setup(v):
    """The store and the two-store table -> the fixture (rows, messages, states, the synchronous results)."""
    z, _ = store_cases.load()
    fin = int(z["store_finalized_slot"])
    runtime.ensure_store(v, fin, z["current_committee"].tobytes(), z["next_committee"].tobytes())
    SM._two_store_table(v, z)
    if "f" in _cache:
        return _cache["f"]
    f = dict(cs=int(z["current_slot"]), gvr=z["genesis_validators_root"].tobytes())
    f["p"] = p = SF.sequence_rows().slice(0, 12)
    f["six"] = six = np.arange(p.n, dtype=np.uint32) % NSTORE
    f["one"] = FoldState(optimistic_slot=fin + 5, current_max_active_participants=200)
    f["two"] = [FoldState(), FoldState(optimistic_slot=fin + 5, previous_max_active_participants=300)]
    f["msgs"] = msgs = WD.wire_messages("finality")[0][:3]
    assert p.n == 12 and len(msgs) == 3
    cs, gvr = f["cs"], f["gvr"]
    assert v.dedup is False
    ok, rs = v.validate(p, cs, gvr)
    f["want_plain"] = (np.asarray(ok, np.uint8), np.asarray(rs, np.uint8))
    ok, rs = v.validate_stores(p, six, cs, gvr)
    f["want_stores"] = (np.asarray(ok, np.uint8), np.asarray(rs, np.uint8))
    ok, rs, res = v.validate_fold(p, cs, gvr, f["one"])
    assert list(np.asarray(ok, np.uint8)) == list(f["want_plain"][0]) and list(rs) == list(f["want_plain"][1])
    f["want_fold"] = res
    ok, rs, res = v.validate_stores_fold(p, six, cs, gvr, f["two"])
    assert list(np.asarray(ok, np.uint8)) == list(f["want_stores"][0]) and list(rs) == list(f["want_stores"][1])
    assert all(r is not None for r in res)
    f["want_stores_fold"] = res
    r = relay_updates(v, msgs, "finality", "deneb", PAIR_ROWS, PAIR_STORES, cs, gvr, dedup=False)
    r.batch.free()
    f["want_relay"] = (np.asarray(r.verdict, np.uint8), np.asarray(r.reason, np.uint8))
    f["want_status"] = (~np.asarray(r.ok, bool)).astype(np.uint8)
    dec, dok = wire.decode_updates_status(msgs, "finality", "deneb", lib=v.lib)
    assert dok.tolist() == np.asarray(r.ok, bool).tolist() and dok.all()
    ok, rs, res = v.validate_stores_fold(SF.take(dec, PAIR_ROWS), PAIR_STORES, cs, gvr, f["two"])
    assert list(np.asarray(ok, np.uint8)) == list(f["want_relay"][0]) and list(rs) == list(f["want_relay"][1])
    f["want_relay_fold"] = res
    # the rows are worth telling apart: accepted and rejected ones, more than one reason
    assert f["want_plain"][0].any() and not f["want_plain"][0].all() and len(set(f["want_plain"][1].tolist())) > 1
    _cache["f"] = f
    return f


def enqueue(v, f, entry, slot=SLOT):
    """-> (rows of the batch, its expected (verdicts, reasons), what must be freed after the waits)."""
    cs, gvr, p, six = f["cs"], f["gvr"], f["p"], f["six"]
    if entry == "validate_resident_async":
        rb = v.upload(p)
        v.validate_resident_async(rb, cs, gvr, slot)
        return p.n, f["want_plain"], rb
    if entry == "validate_async":
        v.validate_async(p, cs, gvr, slot)
        return p.n, f["want_plain"], None
    if entry == "validate_stores_async":
        v.validate_stores_async(p, six, cs, gvr, slot)
        return p.n, f["want_stores"], None
    if entry == "validate_async_fold":
        v.validate_async_fold(p, cs, gvr, f["one"], slot)
        return p.n, f["want_plain"], None
    if entry == "validate_stores_async_fold":
        v.validate_stores_async_fold(p, six, cs, gvr, f["two"], slot)
        return p.n, f["want_stores"], None
    fold_in = f["two"] if entry == "relay_async+fold_in" else None
    v.relay_async(f["msgs"], "finality", "deneb", PAIR_ROWS, PAIR_STORES, cs, gvr, slot, fold_in)
    return len(PAIR_ROWS), f["want_relay"], None


def raw_wait(v, wait, slot, n, nmsg=3):
    """The C wait on sentinel-filled outputs -> (return code, verdicts, reasons, fold results (raw), status bytes)."""
    ver, rea = np.full(max(n, 1), SENTINEL, np.uint8), np.full(max(n, 1), SENTINEL, np.uint8)
    st = np.full(nmsg, SENTINEL, np.uint8)
    res = (FoldResultC * NSTORE)()
    C.memset(res, SENTINEL, C.sizeof(res))
    lib, ctx = v.lib, v.ctx
    if wait == "slot_wait":
        rc = lib.lcv_slot_wait(ctx, slot, n, ptr(ver), ptr(rea))
    elif wait == "slot_wait_fold":
        rc = lib.lcv_slot_wait_fold(ctx, slot, n, ptr(ver), ptr(rea), res)
    elif wait == "slot_wait_stores_fold":
        rc = lib.lcv_slot_wait_stores_fold(ctx, slot, n, ptr(ver), ptr(rea), res)
    else:
        rc = lib.lcv_slot_wait_relay(ctx, slot, ptr(st), ptr(ver), ptr(rea), res if wait.endswith("fold_out") else None)
    return rc, ver[:n], rea[:n], res, st


def untouched(ver, rea, res, st):
    return (ver == SENTINEL).all() and (rea == SENTINEL).all() and (st == SENTINEL).all() and \
        bytes(res) == bytes([SENTINEL]) * C.sizeof(res)


def check_ok_cell(v, f, entry, wait, n, want, got):
    """An OK cell's outputs against the synchronous results of the same rows."""
    rc, ver, rea, res, st = got
    assert rc == OK, (entry, wait, rc, v.lib.lcv_last_error(v.ctx))
    assert ver.tolist() == want[0].tolist() and rea.tolist() == want[1].tolist(), (entry, wait, rea.tolist(), want[1].tolist())
    fold = {"slot_wait_fold": [f["want_fold"]], "slot_wait_stores_fold": f["want_stores_fold"],
            "slot_wait_relay+fold_out": f["want_relay_fold"]}.get(wait)
    if fold is None:
        assert bytes(res) == bytes([SENTINEL]) * C.sizeof(res), (entry, wait)
    else:
        assert v._fold_results(res, range(len(fold)))[:len(fold)] == list(fold), (entry, wait)
        assert all(bytes(res[s]) == bytes([SENTINEL]) * C.sizeof(FoldResultC) for s in range(len(fold), NSTORE))
    if wait.startswith("slot_wait_relay"):
        assert st.tolist() == f["want_status"].tolist(), (entry, wait)
    else:
        assert (st == SENTINEL).all()


def check_entry(v, entry):
    """One row of the table: the batch enqueued on one slot, every cell asserted, the OK waits repeated."""
    f = setup(v)
    n, want, keep = enqueue(v, f, entry)
    try:
        for again in (False, True):  # the second round: a wait does not consume, and a refusal changes nothing
            for wait, code in zip(WAITS, TABLE[entry]):
                got = raw_wait(v, wait, SLOT, n)
                if code == OK:
                    check_ok_cell(v, f, entry, wait, n, want, got)
                else:
                    assert got[0] == ESTATE and untouched(*got[1:]), (entry, wait, again, got[0])
                    assert v.lib.lcv_last_error(v.ctx).decode().startswith("lcv_" + wait.split("+")[0])
        # fewer rows than the batch's: its first rows
        got = raw_wait(v, "slot_wait", SLOT, 5)
        assert got[0] == OK and got[1].tolist() == want[0][:5].tolist() and got[2].tolist() == want[1][:5].tolist()
    finally:
        if keep is not None:
            keep.free()


def check_more_rows_than_the_batch(v):
    """lcv_slot_wait (and the waits that share its row count) refuses n above the batch's rows with LCV_EINVAL and
    writes nothing; the slot's results are still there afterwards."""
    f = setup(v)
    for entry, wait in (("validate_async", "slot_wait"), ("validate_async_fold", "slot_wait_fold"),
                        ("validate_stores_async_fold", "slot_wait_stores_fold"), ("relay_async", "slot_wait")):
        n, want, _ = enqueue(v, f, entry)
        got = raw_wait(v, wait, SLOT, n + 1)
        assert got[0] == EINVAL and untouched(*got[1:]), (entry, wait, got[0])
        assert "more rows than the slot's batch" in v.lib.lcv_last_error(v.ctx).decode()
        check_ok_cell(v, f, entry, wait, n, want, raw_wait(v, wait, SLOT, n))


def check_reuse_by_another_kind(v):
    """A slot reused by a different kind of entry: the old kind's wait then gives LCV_ESTATE, the new kind's its own
    results — through every entry in turn on one slot, and back to the first."""
    f = setup(v)
    order = ENTRIES[::-1] + ENTRIES[-1:] + ENTRIES[:1]
    prev = None
    for entry in order:
        n, want, keep = enqueue(v, f, entry)
        try:
            for wait, code, before in zip(WAITS, TABLE[entry], TABLE[prev] if prev else TABLE[entry]):
                got = raw_wait(v, wait, SLOT, n)
                if code == OK:
                    check_ok_cell(v, f, entry, wait, n, want, got)
                else:
                    assert got[0] == ESTATE and untouched(*got[1:]), (prev, entry, wait, before, got[0])
        finally:
            if keep is not None:
                keep.free()
        prev = entry
    seen = {(a, b) for a, b in zip(order, order[1:])}
    assert any(TABLE[a][k] == OK and TABLE[b][k] == ESTATE for a, b in seen for k in range(1, 5)), "an old kind's wait refused"
