"""Shared cases of the asynchronous-relay tests (tests/test_relay_async_hostsim.py on the host simulation,
tests/test_relay_async_gpu.py on the device): Verifier.relay_async stages wire messages and a (message, store) pair list
into a work-space slot and enqueues decode, fan-out (one kernel, F_wire_relay), validation and, optionally, the
per-store fold; Verifier.slot_wait_relay collects statuses, verdicts, reasons and fold results (include/lcv.h "The
asynchronous relay"); lcv.serving.relay_stream is the serving loop over it.

Expected values never come from the entry under test.  Verdicts and reasons: validate_stores on the host decoder's rows
(lcv.wire.decode_updates_status) tiled on the host, with the deduplication off, and the synchronous
relay_updates(dedup=False), which must agree.  Statuses: the host decoder's and decode_resident's.  Item counts:
relay_updates(dedup=True).dedup.  Fold results: validate_stores_fold on the host-decoded, host-tiled batch.  Everything
is exact bytes: equality, no tolerance.

Fixture: dedup_cases.table_case's update A (valid under store 0) encoded as a finality and as an optimistic message;
the table is table_case's four stores and a fifth whose finalized slot equals A's attested slot.  Every batch has at
most 130 pairs.
"""
import ctypes as C
from dataclasses import asdict

import numpy as np
import pytest

import dedup_cases as D
import dedup_resident_cases as DR
import rlc_cases as R
import store_serving_cases as SV
import store_table_cases as T
import wire_decode_cases as WD
import wire_encode_cases as WE

from lcv import wire
from lcv._native import FoldResultC, FoldStateC, LcvError, RelayRequest, ptr
from lcv.device import FoldState
from lcv.serving import relay_stream, relay_updates

LCV_EINVAL, LCV_ESTATE = -1, -4
KINDS = ("finality", "optimistic")
SHAPES = ((1, 1), (1, 65), (4, 2), (5, 5))  # messages x stores
PAIRS = (1, 63, 64, 65, 130)                # the 64-row seams of the validation's kernels
EXTRA = (0, 1, 31, 32)                      # extra_data lengths: the finalized header at every residue mod 4
NSTORE = 5

_cache = {}


# ------------------------------------------------------------------ the fixture
def fixture(v):
    """-> dict(cs, gvr, A: update A as one packed row); sets the five-store table."""
    case, upd = D.base(v)
    c = T.committees(v)
    fin = case["stores"][0][0]
    a = T.take(upd, [0])
    att_slot = int(a.att_beacon[0, :8].copy().view("<u8")[0])
    rows = [c[0].ssz, c[1].ssz, c[2].ssz, c[0].ssz]
    stores = [(fin, 0, 1), (fin, 0, 1), (fin, 0, D.UNKNOWN), (fin - D.SLOTS_PER_PERIOD, 2, 3), (att_slot, 0, 1)]
    v.set_store_table(np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), T.SC_BYTES), [s[0] for s in stores],
                      [s[1] for s in stores], [s[2] for s in stores])
    return dict(cs=case["current_slot"], gvr=case["gvr"], A=a)


def messages(v, kind, fork="deneb"):
    """Five messages of update A: as it is, and with 0, 1, 31 and 32 bytes of extra_data in the attested header
    (which changes the header: those are rejected, for a reason no store changes)."""
    key = ("msgs", kind, fork)
    if key not in _cache:
        a = fixture(v)["A"]
        p = D.edit(T.take(a, [0] * 5), att_exec=1, att_branch=1, fin_exec=1, fin_branch=1)
        rng = np.random.default_rng(14)
        for j, e in enumerate(EXTRA):
            WE.set_extra(p.att_exec[1 + j], e, rng)
        if fork == "altair":
            for name in ("att_exec", "att_branch", "fin_exec", "fin_branch"):
                getattr(p, name)[:] = 0
        _cache[key] = list(wire.encode_updates(p, kind, fork))
    return _cache[key]


def pair_list(nmsg, nstore):
    """Every message for every store, store by store within a message."""
    rows = np.repeat(np.arange(nmsg, dtype=np.uint32), nstore)
    return rows, np.tile(np.arange(nstore, dtype=np.uint32) % NSTORE, nmsg)


# ------------------------------------------------------------------ the yardsticks
def expected(v, f, msgs, kind, fork, rows, six):
    """(host decoder's ok, (verdicts, reasons)) from the two sources that never run the entry under test."""
    dec, ok = wire.decode_updates_status(msgs, kind, fork, lib=v.lib)
    with D.dedup(v, False):
        want = D.pair(v.validate_stores(T.take(dec, rows), six, f["cs"], f["gvr"]))
        r = relay_updates(v, msgs, kind, fork, rows, six, f["cs"], f["gvr"], dedup=False)
        r.batch.free()
    assert r.ok.tolist() == ok.tolist()
    assert D.same((r.verdict, r.reason), want), (r.reason.tolist(), want[1].tolist())
    return ok, want


def sync_items(v, f, msgs, kind, fork, rows, six, hash_bits=64):
    v.debug_dedup_hash_bits(hash_bits)
    try:
        r = relay_updates(v, msgs, kind, fork, rows, six, f["cs"], f["gvr"], dedup=True)
        r.batch.free()
    finally:
        v.debug_dedup_hash_bits(64)
    return r.dedup


def relay(v, f, msgs, kind, fork, rows, six, slot=0, fold_in=None):
    v.relay_async(msgs, kind, fork, rows, six, f["cs"], f["gvr"], slot, fold_in)
    return v.slot_wait_relay(slot)


def check_modes(v, f, msgs, kind, fork, rows, six, latencies=(0, 64), hash_bits=64, slot=0):
    """The entry with the deduplication off and on, on both engines, against the yardsticks -> (ok, (verdicts, reasons))."""
    ok, want = expected(v, f, msgs, kind, fork, rows, six)
    items = sync_items(v, f, msgs, kind, fork, rows, six, hash_bits)
    assert items[0] == len(rows) and 1 <= items[1] <= len(rows)
    for lat in latencies:
        for mode in (False, True):
            with D.latency(v, lat), D.dedup(v, mode, hash_bits):
                got = relay(v, f, msgs, kind, fork, rows, six, slot)
                dd = v.last_dedup(slot)
            assert got[0].tolist() == ok.tolist(), (lat, mode)
            assert D.same(got[1:3], want), (lat, mode, got[2].tolist(), want[1].tolist())
            assert dd == (items if mode else (len(rows), len(rows))), (lat, mode, dd, items)
    return ok, want


# ------------------------------------------------------------------ 1: parity
def check_fixture(v, kind):
    """All five messages for all five stores: accepted pairs, and pairs rejected for a reason that depends on the store."""
    f = fixture(v)
    msgs = messages(v, kind)
    rows, six = pair_list(5, NSTORE)
    ok, want = check_modes(v, f, msgs, kind, "deneb", rows, six)
    assert ok.all()
    a = want[1][:NSTORE]  # message 0 = A under the five stores
    assert want[0].any() and a[0] == 0 and len(set(a.tolist())) > 1 and (a != 0).any(), a.tolist()
    assert not want[0][NSTORE:].any()  # an edited header is rejected whatever the store


def check_forks(v, kind):
    f = fixture(v)
    per = {fork: messages(v, kind, fork) for fork in WD.FORKS}
    for fork in ("capella", "altair"):
        rows, six = pair_list(2, 2)
        check_modes(v, f, per[fork][:2], kind, fork, rows, six)
    forks = ["deneb", "altair", "capella", "deneb", "capella"]
    msgs = [per[fk][j] for j, fk in enumerate(forks)]
    rows, six = pair_list(5, 2)
    ok, _ = check_modes(v, f, msgs, kind, forks, rows, six)
    assert ok.all()


def check_shape(v, nmsg, nstore):
    f = fixture(v)
    rows, six = pair_list(nmsg, nstore)
    check_modes(v, f, messages(v, "finality")[:nmsg], "finality", "deneb", rows, six)


def check_fan_rows(v):
    """Repeats, a descending run, and message 7 of 8 named by no pair (dedup_resident_cases.FAN_ROWS)."""
    f = fixture(v)
    m = messages(v, "finality")
    msgs = [m[j % 5] for j in range(7)] + [m[1]]
    rows = np.array(DR.FAN_ROWS, np.uint32)
    six = (np.arange(len(rows)) * 3 % NSTORE).astype(np.uint32)
    ok, _ = check_modes(v, f, msgs, "finality", "deneb", rows, six)
    assert ok.all() and 7 not in rows.tolist()


def check_npairs(v, n):
    f = fixture(v)
    msgs = messages(v, "optimistic")[:3]
    rows = (np.arange(n) * 7 % 3).astype(np.uint32)
    six = (np.arange(n) % NSTORE).astype(np.uint32)
    check_modes(v, f, msgs, "optimistic", "deneb", rows, six)


def check_classes(v):
    """Two byte-identical messages are one class; with no hash bits only the full compares separate the classes."""
    f = fixture(v)
    m = messages(v, "finality")
    msgs = [m[0], m[1], m[0], m[2]]
    rows, six = pair_list(4, 3)
    for bits in (64, 0):
        check_modes(v, f, msgs, "finality", "deneb", rows, six, hash_bits=bits)
    # messages 0 and 2 share their items: stores 0, 1, 2 check A's signature against one committee row
    assert sync_items(v, f, [m[0], m[0]], "finality", "deneb", *pair_list(2, 3)) == (6, 1)
    with D.dedup(v, True):
        relay(v, f, [m[0], m[0]], "finality", "deneb", *pair_list(2, 3))
        assert v.last_dedup(0) == (6, 1)


def check_golden(v):
    """The reference-serialised finality messages of tests/golden/wire.npz against the golden store as a one-row table."""
    g = WD.load_updates()
    msgs, _ = WD.wire_messages("finality")
    v.set_store_table(g["nsc_pool"][:2], [int(g["store_finalized_slot"][0])], [0], [1])
    f = dict(cs=int(g["current_slot"][0]), gvr=g["genesis_validators_root"].tobytes())
    rows = np.arange(len(msgs), dtype=np.uint32)
    ok, want = check_modes(v, f, msgs, "finality", "deneb", rows, np.zeros(len(msgs), np.uint32))
    assert ok.all() and want[0].any()


# ------------------------------------------------------------------ 2, 3: malformed messages, unnamed messages
def check_malformed(v):
    f = fixture(v)
    good = messages(v, "finality")[0]
    msgs = [good, good[:WD.FIXED["finality"] - 1], good, good]
    forks = np.array([0, 0, 0, 3], np.uint8)  # (a fork code no name stands for: the raw entry)
    rows = np.array([0, 1, 2, 1, 3, 0], np.uint32)
    six = np.array([0, 1, 2, 3, 0, 3], np.uint32)
    # the yardsticks, through the raw decode entry (per-message codes)
    buf = np.frombuffer(b"".join(msgs), np.uint8)
    lens = np.array([len(m) for m in msgs], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    rc, rb, status = WD.raw_decode(v, buf, offs, lens, 1, 0, forks)
    assert rc == 0 and status.tolist() == [0, 1, 0, 1]
    try:
        with D.dedup(v, False):
            fan = v.fan_out(rb, rows, six)
            try:
                want = D.pair(v.validate_resident(fan, f["cs"], f["gvr"]))
            finally:
                fan.free()
        v.classify_resident(rb)
        fan = v.fan_out(rb, rows, six)
        try:
            with D.dedup(v, True):
                assert D.same(v.validate_resident(fan, f["cs"], f["gvr"]), want)
                items = v.last_dedup()
        finally:
            fan.free()
    finally:
        rb.free()
    assert want[0][[0, 2]].all() and not want[0][[1, 3, 4]].any()
    assert want[1][1] == want[1][3] == want[1][4] != 0  # the zero row's reason
    for mode in (False, True):
        with D.dedup(v, mode):
            st, ver, rea = raw_relay(v, f, buf, offs, lens, 1, 7, forks, rows, six, slot=1)
            assert st.tolist() == status.tolist() and D.same((ver, rea), want), (mode, rea.tolist())
            assert v.last_dedup(1) == (items if mode else (6, 6))


def check_unnamed_status(v):
    f = fixture(v)
    good = messages(v, "optimistic")[0]
    msgs = [good, good[:WD.FIXED["optimistic"] - 1], good]
    ok, want = expected(v, f, msgs, "optimistic", "deneb", [0, 0], [0, 3])
    got = relay(v, f, msgs, "optimistic", "deneb", [0, 0], [0, 3])
    assert got[0].tolist() == ok.tolist() == [True, False, True] and D.same(got[1:3], want)


# ------------------------------------------------------------------ the raw entry
def request(f, msg_buf, offs, lens, kind_code, fork_code, codes, pair_rows, six, states=None, **over):
    """(lcv_relay_request with the fields of `over` replaced, the arrays it points into)."""
    keep = dict(buf=np.ascontiguousarray(msg_buf, np.uint8), offs=np.ascontiguousarray(offs, np.uint64),
                lens=np.ascontiguousarray(lens, np.uint64), rows=np.ascontiguousarray(pair_rows, np.uint32),
                six=np.ascontiguousarray(six, np.uint32), gvr=np.frombuffer(bytes(f["gvr"]), np.uint8),
                forks=None if codes is None else np.ascontiguousarray(codes, np.uint8))
    a = dict(buf=ptr(keep["buf"]), buf_len=keep["buf"].size, offsets=ptr(keep["offs"], C.c_uint64),
             lengths=ptr(keep["lens"], C.c_uint64), nmsg=keep["offs"].size, kind=kind_code, fork=fork_code,
             forks=None if codes is None else ptr(keep["forks"]), rows=ptr(keep["rows"], C.c_uint32),
             store_index=ptr(keep["six"], C.c_uint32), npairs=keep["rows"].size, current_slot=f["cs"],
             genesis_validators_root=ptr(keep["gvr"]), fold_in=states)
    keep["over"] = over
    a.update(over)
    return RelayRequest(**a), keep


def raw_relay(v, f, buf, offs, lens, kind, fork, forks, rows, six, slot=0):
    rq, keep = request(f, buf, offs, lens, kind, fork, forks, rows, six)
    assert v.lib.lcv_relay_async(v.ctx, C.byref(rq), slot) == 0, v.lib.lcv_last_error(v.ctx)
    st, ver, rea = np.full(len(offs), 0xEE, np.uint8), np.full(len(rows), 0xEE, np.uint8), np.full(len(rows), 0xEE, np.uint8)
    assert v.lib.lcv_slot_wait_relay(v.ctx, slot, ptr(st), ptr(ver), ptr(rea), None) == 0
    return st, ver.astype(bool), rea


# ------------------------------------------------------------------ 4: eight in flight
def check_slots(v):
    f = fixture(v)
    m = {k: messages(v, k) for k in KINDS}
    reqs = []
    for s in range(8):
        kind = KINDS[s % 2]
        nmsg = 1 + s % 5
        rows = (np.arange(3 + 2 * s) * 3 % nmsg).astype(np.uint32)
        six = ((np.arange(3 + 2 * s) + s) % NSTORE).astype(np.uint32)
        reqs.append((m[kind][:nmsg], kind, "deneb", rows, six))
    want = [expected(v, f, *r) for r in reqs]
    big = (m["finality"], "finality", "deneb", *pair_list(5, 26))
    want_big = expected(v, f, *big)
    pool0 = v.event_pool()

    def right(got, w):
        return got[0].tolist() == w[0].tolist() and D.same(got[1:3], w[1])

    with D.dedup(v, True):
        for s, r in enumerate(reqs):
            v.relay_async(*r, f["cs"], f["gvr"], s)
        for s in reversed(range(8)):
            assert right(v.slot_wait_relay(s), want[s]), s
        # slot 3 again: smaller, larger (its buffers regrow while the other slots are busy), equal
        for s in (0, 1, 2, 4, 5, 6, 7):
            v.relay_async(*reqs[s], f["cs"], f["gvr"], s)
        for r, w in ((reqs[0], want[0]), (big, want_big), (big, want_big)):
            v.relay_async(*r, f["cs"], f["gvr"], 3)
            assert right(v.slot_wait_relay(3), w)
        for s in (7, 6, 5, 4, 2, 1, 0):
            assert right(v.slot_wait_relay(s), want[s]), s
    assert v.event_pool() <= max(pool0, 64)


# ------------------------------------------------------------------ 5: mixed traffic
def check_mixed_traffic(v):
    f = fixture(v)
    msgs = messages(v, "finality")[:2]
    rows, six = pair_list(2, NSTORE)
    ok, want = expected(v, f, msgs, "finality", "deneb", rows, six)
    p = T.take(f["A"], [0] * NSTORE)
    index = np.arange(NSTORE, dtype=np.uint32)
    with D.dedup(v, False):
        want_p = D.pair(v.validate_stores(p, index, f["cs"], f["gvr"]))
    for relay_first in (True, False):
        v.validate_stores_async(p, index, f["cs"], f["gvr"], 2)
        v.relay_async(msgs, "finality", "deneb", rows, six, f["cs"], f["gvr"], 6)
        if relay_first:
            got = v.slot_wait(6, len(rows))  # the plain wait hands out a relay slot's verdicts
            assert D.same(got, want)
        assert D.same(v.slot_wait(2, p.n), want_p)
        got = v.slot_wait_relay(6)
        assert got[0].tolist() == ok.tolist() and D.same(got[1:3], want)
        # the other entries' waits refuse a relay slot, and the relay's wait a plain slot
        res = (FoldResultC * NSTORE)()
        out = np.zeros(len(rows), np.uint8)
        assert v.lib.lcv_slot_wait_fold(v.ctx, 6, len(rows), ptr(out), ptr(out), res) == LCV_ESTATE
        assert v.lib.lcv_slot_wait_stores_fold(v.ctx, 6, len(rows), ptr(out), ptr(out), res) == LCV_ESTATE
        assert v.lib.lcv_slot_wait_relay(v.ctx, 2, None, ptr(out), ptr(out), None) == LCV_ESTATE
        assert "not enqueued by lcv_relay_async" in v.lib.lcv_last_error(v.ctx).decode()


# ------------------------------------------------------------------ 6: the fold
def fold_expected(v, f, msgs, kind, rows, six, states):
    dec, _ = wire.decode_updates_status(msgs, kind, "deneb", lib=v.lib)
    with D.dedup(v, False):
        return v.validate_stores_fold(T.take(dec, rows), six, f["cs"], f["gvr"], states)


def same_fold(got, want):
    return [None if r is None else asdict(r) for r in got] == [None if r is None else asdict(r) for r in want]


def check_fold(v):
    f = fixture(v)
    m = messages(v, "finality")
    states = [FoldState() for _ in range(NSTORE)]
    states[1] = FoldState(optimistic_slot=3, previous_max_active_participants=400, current_max_active_participants=17)
    lists = [(m, *pair_list(5, NSTORE)),
             # 3 messages x 4 stores, the stores interleaved; store 4 is absent
             ([m[0], m[1], m[0]], np.array([0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 1, 2], np.uint32),
              np.array([3, 0, 1, 2, 0, 3, 1, 0, 2, 1, 2, 3], np.uint32))]
    for msgs, rows, six in lists:
        want = fold_expected(v, f, msgs, "finality", rows, six, states)
        for mode in (False, True):
            with D.dedup(v, mode):
                got = relay(v, f, msgs, "finality", "deneb", rows, six, slot=4, fold_in=states)
            assert D.same(got[1:3], want[:2]) and same_fold(got[3], want[2]), mode
    assert want[2][4] is None and all(r is not None for r in want[2][:4])
    assert any(r.apply_row >= 0 for r in want[2][:4]), [r.apply_row for r in want[2][:4]]
    # absent stores' entries are untouched; a wait for fold results of a relay without fold_in is refused
    msgs, rows, six = lists[1]
    v.relay_async(msgs, "finality", "deneb", rows, six, f["cs"], f["gvr"], 4, states)
    res = (FoldResultC * NSTORE)()
    C.memset(res, 0xA5, C.sizeof(res))
    out = np.zeros(len(rows), np.uint8)
    assert v.lib.lcv_slot_wait_relay(v.ctx, 4, None, ptr(out), ptr(out), res) == 0
    assert bytes(res[4]) == b"\xa5" * C.sizeof(FoldResultC) and bytes(res[3]) != b"\xa5" * C.sizeof(FoldResultC)
    v.relay_async(msgs, "finality", "deneb", rows, six, f["cs"], f["gvr"], 4)
    assert v.lib.lcv_slot_wait_relay(v.ctx, 4, None, ptr(out), ptr(out), res) == LCV_ESTATE
    assert "without fold_in" in v.lib.lcv_last_error(v.ctx).decode()
    assert v.lib.lcv_slot_wait_relay(v.ctx, 4, None, ptr(out), ptr(out), None) == 0


# ------------------------------------------------------------------ 7: batch verification
def check_rlc(v):
    f = fixture(v)
    msgs = messages(v, "finality")
    rows, six = pair_list(5, NSTORE)
    ok, want = expected(v, f, msgs, "finality", "deneb", rows, six)
    with D.latency(v, 0), R.rlc(v, 8, R.SEED):
        for mode in (False, True):
            with D.dedup(v, mode):
                got = relay(v, f, msgs, "finality", "deneb", rows, six, slot=5)
            assert got[0].tolist() == ok.tolist() and D.same(got[1:3], want), mode
            assert v.last_rlc(5)[0] > 0


# ------------------------------------------------------------------ 8: refusals
def check_refusals(v, fresh):
    """`fresh`: a context of v's backend with no table set and no relay enqueued."""
    f = fixture(v)
    lib, ctx = v.lib, v.ctx
    msgs = messages(v, "finality")[:3]
    buf = np.frombuffer(b"".join(msgs), np.uint8)
    lens = np.array([len(x) for x in msgs], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    rows, six = np.array([0, 1, 2, 1], np.uint32), np.array([0, 1, 2, 4], np.uint32)
    slot = 7
    # the slot's last batch is no relay, so a refusal that enqueued nothing leaves lcv_slot_wait_relay refusing
    p = T.take(f["A"], [0])
    v.validate_stores_async(p, [0], f["cs"], f["gvr"], slot)
    v.slot_wait(slot, 1)
    v.engine_log(reset=True)

    def refused(status=LCV_EINVAL, c=None, s=slot, rq=True, fold_in=None, **over):
        r, keep = request(f, buf, offs, lens, 1, 0, None, rows, six, fold_in, **over)
        rc = lib.lcv_relay_async(ctx if c is None else c, C.byref(r) if rq else None, s)
        assert rc == status, (rc, over)
        err = lib.lcv_last_error(ctx if c is None else c).decode()
        out = np.zeros(4, np.uint8)
        assert lib.lcv_slot_wait_relay(ctx, slot, None, ptr(out), ptr(out), None) == LCV_ESTATE
        log = v.engine_log()
        assert log["fan"] == log["batch"] == log["twin"] == log["lane"] == 0
        return err

    assert lib.lcv_relay_async(None, None, 0) == LCV_EINVAL
    assert "null" in refused(rq=False)
    for name in ("buf", "offsets", "lengths", "rows", "store_index", "genesis_validators_root"):
        assert "null" in refused(**{name: None}), name
    assert "slot" in refused(s=8) and "slot" in refused(s=-1)
    for kind in (0, 3, -1):
        assert "kind" in refused(kind=kind)
    assert "fork" in refused(fork=3) and "fork" in refused(fork=-1)
    assert "nmsg > 0" in refused(nmsg=0) and "npairs > 0" in refused(npairs=0)
    big = np.zeros(65537, np.uint64)
    assert "LCV_DECODE_MAX_ROWS" in refused(nmsg=65537, offsets=ptr(big, C.c_uint64), lengths=ptr(big, C.c_uint64))
    with SV.chunk(v, 3):
        assert "npairs = 4" in refused()
    for o, ln in ((int(offs[2]), int(lens[2]) + 1), (buf.size, 1), (2 ** 64 - 1, 2), (1, 2 ** 64 - 1), (2 ** 63, 2 ** 63)):
        o3, l3 = offs.copy(), lens.copy()
        o3[2], l3[2] = o, ln
        err = refused(offsets=ptr(o3, C.c_uint64), lengths=ptr(l3, C.c_uint64))
        assert "message 2" in err and "buf_len" in err, (o, ln, err)
    # staged bytes: 8193 entries naming one 32 KiB window are staged 8193 times (256 MiB and more)
    win = np.zeros(32768, np.uint8)
    err = refused(buf=ptr(win), buf_len=win.size, nmsg=8193, offsets=ptr(np.zeros(8193, np.uint64), C.c_uint64),
                  lengths=ptr(np.full(8193, 32768, np.uint64), C.c_uint64))
    assert "LCV_RELAY_MAX_BYTES" in err and "message 8191" in err, err
    assert "rows[2] = 3" in refused(rows=ptr(np.array([0, 1, 3, 9], np.uint32), C.c_uint32))
    assert "store_index[3] = 5" in refused(store_index=ptr(np.array([0, 1, 2, 5], np.uint32), C.c_uint32))
    states = (FoldStateC * NSTORE)()
    states[4].current_max_active_participants = 513  # store 4 is present (pair 3)
    assert "in[4]" in refused(fold_in=states)
    states[4].current_max_active_participants = 0
    states[3].previous_max_active_participants = 513  # store 3 is absent: its state is not looked at
    r, keep = request(f, buf, offs, lens, 1, 0, None, rows, six, states)
    assert lib.lcv_relay_async(ctx, C.byref(r), 0) == 0 and len(v.slot_wait(0, 4)[0]) == 4
    v.engine_log(reset=True)
    with SV.pipeline(v, 2, 2):
        assert "multi-stream pipeline" in refused()
    # no table
    r, keep = request(f, buf, offs, lens, 1, 0, None, rows, six)
    assert fresh.lib.lcv_relay_async(fresh.ctx, C.byref(r), 0) == LCV_ESTATE
    assert "lcv_set_store_table" in fresh.lib.lcv_last_error(fresh.ctx).decode()
    assert fresh.lib.lcv_slot_wait_relay(fresh.ctx, 0, None, None, None, None) == LCV_ESTATE
    assert lib.lcv_slot_wait_relay(ctx, 8, None, None, None, None) == LCV_EINVAL
    assert lib.lcv_last_relay_timings(ctx, 0, None) == LCV_EINVAL
    with pytest.raises(LcvError, match=f"status {LCV_EINVAL}"):
        v.relay_async(msgs, "update", "deneb", rows, six, f["cs"], f["gvr"], 0)
    # the entry still works, and its kernel was timed
    got = relay(v, f, msgs, "finality", "deneb", rows, six, slot=slot)
    assert got[0].all() and v.last_relay_timings(slot)[0] > 0 and v.last_relay_timings(slot)[1] == 0.0


# ------------------------------------------------------------------ 9: the serving loop
def check_stream(v, in_flight):
    f = fixture(v)
    m = {k: messages(v, k) for k in KINDS}
    items = []
    for j in range(10):
        kind = KINDS[j % 2]
        nmsg = 1 + j % 4
        rows = (np.arange(2 + j) * 5 % nmsg).astype(np.uint32)
        items.append((m[kind][:nmsg], kind, "deneb", rows, ((np.arange(2 + j) + j) % NSTORE).astype(np.uint32)))
    key = "stream"
    if key not in _cache:  # ten synchronous relays, once
        want = []
        for it in items:
            r = relay_updates(v, *it, f["cs"], f["gvr"], dedup=True)
            r.batch.free()
            want.append(r)
        _cache[key] = want
    want = _cache[key]
    for before in (False, True):
        v.set_dedup(before)
        try:
            got = list(relay_stream(v, iter(items), f["cs"], f["gvr"], in_flight=in_flight))
            assert v.dedup is before
        finally:
            v.set_dedup(False)
        assert len(got) == 10
        for g, w in zip(got, want):
            assert g.ok.tolist() == w.ok.tolist() and D.same((g.verdict, g.reason), (w.verdict, w.reason)) and g.dedup == w.dedup
    # a bad item: the error surfaces, nothing stays in flight, the setting is restored
    bad = items[:3] + [(items[3][0], "finality", "deneb", [9], [0])] + items[4:]
    with pytest.raises(LcvError, match="rows"):
        list(relay_stream(v, iter(bad), f["cs"], f["gvr"], in_flight=in_flight))
    assert v.dedup is False
    with pytest.raises(ValueError):
        list(relay_stream(v, iter(items), f["cs"], f["gvr"], in_flight=9))
    states = [FoldState() for _ in range(NSTORE)]
    got = list(relay_stream(v, iter(items[:2]), f["cs"], f["gvr"], in_flight=in_flight, fold_states=states))
    for g, it in zip(got, items[:2]):
        assert same_fold(g.fold, fold_expected(v, f, it[0], it[1], it[3], it[4], states)[2])
