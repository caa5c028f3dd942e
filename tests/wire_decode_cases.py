"""Cases and checks of the device SSZ decoder (lcv_batch_decode, Verifier.decode_resident,
lcv.wire.decode_updates_device), shared by test_wire_decode_hostsim.py (host simulation of the kernels' code) and
test_wire_decode_gpu.py (the MI355X).

The yardstick is the host decoder (lcv_ssz_decode_updates / _mixed, csrc/lcv_wire.cpp), which tests/test_wire.py pins
to the reference-serialised messages of tests/golden/wire.npz.  Messages are those, an Altair update serialised by the
oracle's SSZ, and lcv.wire.encode_updates over the generated rows of wire_encode_cases.  Every batch has at most 130
messages of at most 27 KB.
"""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest

import helpers as H
import wire_encode_cases as WE
from golden_cases import COLS, GOLDEN, load_updates

from lcv import wire
from lcv._native import LcvError, ptr
from lcv.device import PackedUpdates

KINDS, FORKS = WE.KINDS, WE.FORKS
ALL_COLS = COLS + ("nsc_index", "signature_slot", "nsc_pool")
SC = 24624
FIXED = {"update": 25152, "finality": 368, "optimistic": 172}
ALTAIR_SIZE = {"update": 25368, "finality": 584, "optimistic": 280}
EXEC_FIXED = {"deneb": 584, "capella": 568}


def load_wire():
    return dict(np.load(os.path.join(GOLDEN, "wire.npz"), allow_pickle=False))


def wire_messages(kind):
    w = load_wire()
    sel = np.flatnonzero(w["kind"] == KINDS.index(kind))
    return [w["buf"][int(w["offsets"][i]):int(w["offsets"][i] + w["lengths"][i])].tobytes() for i in sel], w["row"][sel]


def assert_batches_equal(got, exp, what=""):
    for k in ALL_COLS:
        a, b = getattr(got, k), getattr(exp, k)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if not np.array_equal(a, b):
            rows = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
            raise AssertionError(f"{what}: column {k} differs in rows {rows[:8].tolist()}")


def decode_both(v, msgs, kind, fork):
    """(device rows downloaded, device ok, host rows, host ok) of the same messages."""
    exp, eok = wire.decode_updates_status(msgs, kind, fork, lib=v.lib)
    rb, ok = v.decode_resident(msgs, kind, fork)
    try:
        assert rb.n == exp.n and rb.npool == exp.nsc_pool.shape[0], (rb.n, rb.npool, exp.nsc_pool.shape)
        got = v.download(rb)
    finally:
        rb.free()
    return got, ok, exp, eok


def assert_same_as_host(v, msgs, kind, fork, what=""):
    got, ok, exp, eok = decode_both(v, msgs, kind, fork)
    assert ok.tolist() == eok.tolist(), (what, ok.tolist(), eok.tolist())
    assert_batches_equal(got, exp, what)
    return got, ok


def altair_update():
    p = WE.packed()
    u = H.update_from(p, 30)  # bellatrix_valid: pre-Capella, empty execution
    return WE.serialize(WE.AltairUpdate(attested_header=WE.AltairHeader(beacon=u.attested_header.beacon),
                                        next_sync_committee=u.next_sync_committee,
                                        next_sync_committee_branch=u.next_sync_committee_branch,
                                        finalized_header=WE.AltairHeader(beacon=u.finalized_header.beacon),
                                        finality_branch=u.finality_branch, sync_aggregate=u.sync_aggregate,
                                        signature_slot=u.signature_slot))


# ------------------------------------------------------------------ 1. reference bytes
def check_reference_bytes(v):
    for kind in KINDS:
        msgs, _ = wire_messages(kind)
        assert msgs
        got, ok = assert_same_as_host(v, msgs, kind, "deneb", kind)
        assert ok.all()
        got.check()
    alt = altair_update()
    assert len(alt) == ALTAIR_SIZE["update"]
    got, ok = assert_same_as_host(v, [alt], "update", "altair", "altair")
    assert ok.all() and not got.att_exec.any() and got.nsc_pool[got.nsc_index[0]].any()


# ------------------------------------------------------------------ 2. differential against the host decoder
@lru_cache(maxsize=None)
def encoded(n, kind, fork):
    return tuple(wire.encode_updates(WE.rows_for(n, fork), kind, fork))


def check_differential(v, kind, fork, n):
    msgs = list(encoded(n, kind, fork))
    got, ok = assert_same_as_host(v, msgs, kind, fork, f"{kind}/{fork}/{n}")
    assert ok.all()
    if fork != "altair" and kind != "optimistic" and n >= 33:  # the finalized header starts at all 16 residues
        att, _ = WE.elens(WE.rows_for(n, fork))
        assert {(FIXED[kind] + 244 + EXEC_FIXED[fork] + a) % 16 for a in att.tolist()} == set(range(16))


def mixed_messages(kind, n=130):
    forks = [FORKS[j % 3] for j in range(n)]
    per = {f: encoded(n, kind, f) for f in FORKS}
    return [per[f][j] for j, f in enumerate(forks)], forks


def check_mixed_forks(v, kind):
    msgs, forks = mixed_messages(kind)
    _, ok = assert_same_as_host(v, msgs, kind, forks, f"mixed {kind}")
    assert ok.all()
    # the fork decides the layout: every message under its neighbour's fork
    wrong = forks[1:] + forks[:1]
    _, ok = assert_same_as_host(v, msgs, kind, wrong, f"mixed {kind}, wrong forks")
    assert ok.tolist() == [f == w for f, w in zip(forks, wrong)] and not ok[:-1].any()


# ------------------------------------------------------------------ 3. round trip on the device
def check_round_trip(v, kind, fork, n=130):
    msgs = list(encoded(n, kind, fork))
    rb, ok = wire.decode_updates_device(msgs, kind, fork, verifier=v)
    try:
        assert ok.all()
        enc = v.encode_resident(rb, kind, fork)
    finally:
        rb.free()
    WE.assert_encoded(enc, msgs, FORKS.index(fork))


# ------------------------------------------------------------------ 4. the malformed table
def with_u32(b, pos, value):
    return b[:pos] + int(value & 0xFFFFFFFF).to_bytes(4, "little") + b[pos + 4:]


@lru_cache(maxsize=None)
def long_message(kind, fork):
    """A message of the greatest length its kind and fork have: 32 bytes of extra_data in every header."""
    b = WE.take(WE.rows_for(1, fork), [0])
    rng = np.random.default_rng(5)
    if fork != "altair":
        WE.set_extra(b.att_exec[0], 32, rng)
        WE.set_extra(b.fin_exec[0], 32, rng)
    return wire.encode_updates(b, kind, fork)[0]


@lru_cache(maxsize=None)
def malformed_table(kind, fork):
    """(good message, [(name, bad message)])."""
    good = long_message(kind, fork)
    n = len(good)
    if fork == "altair":
        assert n == ALTAIR_SIZE[kind]
        return good, [("empty", b""), ("altair length - 1", good[:-1]), ("altair length + 1", good + b"\0")]
    fixed, ef = FIXED[kind], EXEC_FIXED[fork]
    hdr = 244 + ef + 32
    two = kind != "optimistic"
    assert n == fixed + (2 if two else 1) * hdr
    pos2 = {"update": 4 + SC + 160, "finality": 4}.get(kind)  # where the second offset stands
    bad = [("empty", b""), ("one byte short of the fixed part", good[:fixed - 1]),
           ("first offset + 1", with_u32(good, 0, fixed + 1)), ("first offset - 1", with_u32(good, 0, fixed - 1)),
           ("inner offset != 244", with_u32(good, fixed + 112, 245)),
           ("extra_data offset field", with_u32(good, fixed + 244 + 436, ef + 4)),
           ("extra_data of 33 bytes", good + b"\x07"), ("length max + 1", good + b"\0"),
           ("fixed part only", good[:fixed])]
    if two:
        bad += [("second offset below the first", with_u32(good, pos2, fixed - 1)),
                ("second offset = len + 1", with_u32(good, pos2, n + 1)),
                ("second offset = 0x80000000", with_u32(good, pos2, 0x80000000)),
                ("second offset = 0xFFFFFFFF", with_u32(good, pos2, 0xFFFFFFFF)),
                ("second offset = len (an empty header)", with_u32(good, pos2, n)),
                ("attested header of 243 bytes", with_u32(good, pos2, fixed + 243)),
                ("finalized header of 243 bytes", good[:fixed + hdr + 243]),
                ("attested execution header one byte short", with_u32(good, pos2, fixed + 244 + ef - 1)),
                ("finalized execution header one byte short", good[:fixed + hdr + 244 + ef - 1]),
                ("finalized inner offset != 244", with_u32(good, fixed + hdr + 112, 243)),
                ("finalized extra_data offset field", with_u32(good, fixed + hdr + 244 + 436, ef - 1)),
                ("attested extra_data of 33 bytes", with_u32(good, pos2, fixed + hdr + 1))]
    else:
        bad += [("header of 243 bytes", good[:fixed + 243]),
                ("execution header one byte short", good[:fixed + 244 + ef - 1])]
    return good, bad


def all_zero(batch, i):
    return not any(getattr(batch, k)[i].any() for k in COLS + ("signature_slot",))


def check_malformed(v, kind, fork):
    good, bad = malformed_table(kind, fork)
    alone, ok = assert_same_as_host(v, [good], kind, fork, "the good message")
    assert ok.all() and not all_zero(alone, 0)
    msgs = [good]
    for _, b in bad:
        msgs += [b, good]
    got, ok = assert_same_as_host(v, msgs, kind, fork, f"table {kind}/{fork}")
    assert ok.tolist() == [j % 2 == 0 for j in range(len(msgs))], [name for (name, _), o in zip(bad, ok[1::2]) if o]
    for j in range(len(msgs)):
        if j % 2:
            assert all_zero(got, j), bad[j // 2][0]
        else:
            for k in COLS + ("signature_slot",):
                assert np.array_equal(getattr(got, k)[j], getattr(alone, k)[0]), (j, k)
            assert np.array_equal(got.nsc_pool[got.nsc_index[j]], alone.nsc_pool[alone.nsc_index[0]])
    # each bad message as the first and as the last message of the buffer
    for name, b in bad:
        for pair, exp_ok in (([b, good], [False, True]), ([good, b], [True, False])):
            got, ok = assert_same_as_host(v, pair, kind, fork, name)
            assert ok.tolist() == exp_ok, name
            assert all_zero(got, exp_ok.index(False)), name
    # a good batch decoded and freed, then an all-malformed batch of the same n
    n = len(bad)
    rb, ok = v.decode_resident([good] * n, kind, fork)
    assert ok.all()
    rb.free()
    got, ok = assert_same_as_host(v, [b for _, b in bad], kind, fork, "all malformed")
    assert not ok.any() and all(all_zero(got, i) for i in range(n))
    assert got.nsc_pool.shape[0] == 1 and not got.nsc_pool.any() and not got.nsc_index.any()
    with pytest.raises(ValueError, match=r"index \[1, 3"):
        wire.decode_updates_device(msgs, kind, fork, verifier=v)
    rb, ok = wire.decode_updates_device(msgs, kind, fork, verifier=v, strict=False)
    rb.free()
    assert ok.tolist() == [j % 2 == 0 for j in range(len(msgs))]


def raw_decode(v, buf, offs, lens, kind, fork, codes=None):
    """lcv_batch_decode itself -> (rc, ResidentBatch or None, status)."""
    from lcv.device import ResidentBatch
    n = len(offs)
    buf = np.ascontiguousarray(buf, np.uint8)
    offs, lens = np.ascontiguousarray(offs, np.uint64), np.ascontiguousarray(lens, np.uint64)
    status = np.full(max(n, 1), 0xEE, np.uint8)
    h = C.c_void_p()
    rc = v.lib.lcv_batch_decode(v.ctx, ptr(buf), buf.size, ptr(offs, C.c_uint64), ptr(lens, C.c_uint64), n, kind, fork,
                                None if codes is None else ptr(codes), ptr(status), C.byref(h))
    if rc != 0 or not h:
        return rc, None, status
    rows, npool = C.c_uint64(), C.c_uint64()
    assert v.lib.lcv_batch_shape(v.ctx, h, C.byref(rows), C.byref(npool)) == 0 and rows.value == n
    return rc, ResidentBatch(v, h, n, npool=int(npool.value)), status


def check_fork_code_3(v, kind):
    """A fork code outside 0..2 in a per-message list: status 1 and an all-zero row, as the host decoder gives."""
    msgs, forks = mixed_messages(kind, 9)
    codes = np.array([FORKS.index(f) for f in forks], np.uint8)
    codes[[0, 4, 8]] = 3, 255, 3
    buf = np.frombuffer(b"".join(msgs), np.uint8)
    lens = np.array([len(m) for m in msgs], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    exp = PackedUpdates.empty(9, 10)
    b, keep = exp.to_c()
    pool_src, npool, st = np.zeros(10, np.uint64), C.c_uint64(), np.zeros(9, np.uint8)
    assert v.lib.lcv_ssz_decode_updates_mixed(ptr(buf), ptr(offs, C.c_uint64), ptr(lens, C.c_uint64), 9, KINDS.index(kind),
                                             ptr(codes), C.byref(b), ptr(pool_src, C.c_uint64), C.byref(npool), ptr(st)) == 0
    assert st.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    rc, rb, status = raw_decode(v, buf, offs, lens, KINDS.index(kind), 7, codes)  # (`fork` is ignored)
    assert rc == 0 and status.tolist() == st.tolist()
    try:
        got = v.download(rb)
    finally:
        rb.free()
    for k in COLS + ("signature_slot",):
        assert np.array_equal(getattr(got, k), getattr(exp, k)), k
    for i in range(9):
        s = int(pool_src[exp.nsc_index[i]])
        committee = bytes(SC) if s == 0xFFFFFFFFFFFFFFFF else buf[s:s + SC].tobytes()
        assert got.nsc_pool[got.nsc_index[i]].tobytes() == committee, i
    assert all(all_zero(got, i) for i in (0, 4, 8))


# ------------------------------------------------------------------ 5. buffer forms
def check_buffer_forms(v, kind="update", fork="deneb"):
    msgs = list(encoded(5, kind, fork))
    rng = np.random.default_rng(3)
    order = [4, 2, 3, 0, 1]  # descending and mixed offsets; the last message of buf is listed first
    parts, offs, pos = [], {}, 0
    for j in range(5):
        gap = bytes(rng.integers(1, 256, 1 + 5 * j, dtype=np.uint8)) if j else b""
        parts += [gap, msgs[j]]
        pos += len(gap)
        offs[j] = pos
        pos += len(msgs[j])
    buf = np.frombuffer(b"".join(parts), np.uint8)
    assert offs[4] + len(msgs[4]) == buf.size  # a message that ends at buf_len exactly
    listed = order + [2, 4]                    # two entries naming the same bytes
    o = np.array([offs[j] for j in listed], np.uint64)
    ln = np.array([len(msgs[j]) for j in listed], np.uint64)
    got, ok = assert_same_as_host(v, (buf, o, ln), kind, fork, "tuple form")
    assert ok.all()
    ref, _ = assert_same_as_host(v, [msgs[j] for j in listed], kind, fork, "list form")
    assert_batches_equal(got, ref, "tuple against list")
    # overlapping entries: a window inside a message is just another (malformed) message
    o2 = np.array([offs[0], offs[0] + 8, offs[0]], np.uint64)
    l2 = np.array([len(msgs[0]), len(msgs[0]) - 8, len(msgs[0])], np.uint64)
    _, ok = assert_same_as_host(v, (buf, o2, l2), kind, fork, "overlap")
    assert ok.tolist() == [True, False, True]


# ------------------------------------------------------------------ 6. the pool
def first_occurrence_pool(msgs, fork="deneb"):
    """(nsc_index, pool rows) by content in order of first occurrence, from a dict of bytes."""
    at = 112 if fork == "altair" else 4
    seen, index = {}, []
    for m in msgs:
        index.append(seen.setdefault(m[at:at + SC], len(seen)))
    return index, list(seen)


def with_committee(m, committee):
    return m[:4] + committee + m[4 + SC:]


def check_pool(v):
    msgs, _ = wire_messages("update")
    got, ok = assert_same_as_host(v, msgs * 5, "update", "deneb", "five times")
    assert ok.all() and got.nsc_pool.shape[0] <= 3
    index, pool = first_occurrence_pool(msgs * 5)
    assert got.nsc_index.tolist() == index and [r.tobytes() for r in got.nsc_pool] == pool
    assert v.last_decode_timings()[1] > 0
    # SyncCommittee() takes a pool row at its first use
    base = list(encoded(6, "update", "deneb"))
    zero = with_committee(base[0], bytes(SC))
    for at in (0, 3):
        m = base[:at] + [zero] + base[at:]
        got, ok = assert_same_as_host(v, m, "update", "deneb", f"zero committee at {at}")
        index, pool = first_occurrence_pool(m)
        assert ok.all() and got.nsc_index.tolist() == index and [r.tobytes() for r in got.nsc_pool] == pool
        assert not got.nsc_pool[got.nsc_index[at]].any()
    # three distinct committees and the zero one under whole, one-bit and no hash: only the full compare separates
    rng = np.random.default_rng(11)
    c0 = base[0][4:4 + SC]
    mid = bytearray(c0)
    mid[48 * 200 + 7] ^= 0x40       # differs from c0 in one byte far from both ends
    last = bytearray(c0)
    last[SC - 1] ^= 0x01            # ... in its last byte
    comms = [c0, bytes(mid), bytes(last), bytes(SC)]
    pick = [2, 0, 1, 0, 3, 2, 1, 1, 3, 0, 2] + rng.integers(0, 4, 30).tolist()
    m = [with_committee(base[j % 6], comms[c]) for j, c in enumerate(pick)]
    index, pool = first_occurrence_pool(m)
    assert len(pool) == 4
    try:
        runs = []
        for bits in (64, 1, 0):
            v.debug_decode_hash_bits(bits)
            rb, ok = v.decode_resident(m, "update", "deneb")
            try:
                assert ok.all() and rb.npool == 4
                runs.append(v.download(rb))
            finally:
                rb.free()
            assert v.last_decode_timings()[1] > 0
    finally:
        v.debug_decode_hash_bits(64)
    for got in runs:
        assert got.nsc_index.tolist() == index and [r.tobytes() for r in got.nsc_pool] == pool
        assert_batches_equal(got, runs[0], "hash bits")
    # only updates have a pool to resolve
    for kind in ("finality", "optimistic"):
        rb, ok = v.decode_resident(list(encoded(5, kind, "deneb")), kind, "deneb")
        rb.free()
        t = v.last_decode_timings()
        assert ok.all() and t[0] > 0 and t[1] == 0.0, (kind, t)
    with pytest.raises(LcvError, match="status -1"):
        v.debug_decode_hash_bits(65)


# ------------------------------------------------------------------ 7. validate where it lies
def check_validate(v):
    g = load_updates()
    gvr = g["genesis_validators_root"].tobytes()
    cur, nxt = g["nsc_pool"][0].tobytes(), g["nsc_pool"][1].tobytes()
    v.set_store(int(g["store_finalized_slot"][0]), cur, nxt)
    cs = int(g["current_slot"][0])
    for kind in KINDS:
        msgs, _ = wire_messages(kind)
        exp_ok, exp_reason = v.validate(wire.decode_updates(msgs, kind, lib=v.lib), cs, gvr)
        rb, ok = v.decode_resident(msgs, kind)
        try:
            assert ok.all()
            got_ok, got_reason = v.validate_resident(rb, cs, gvr)
        finally:
            rb.free()
        assert got_reason.tolist() == exp_reason.tolist() and got_ok.tolist() == exp_ok.tolist(), kind
        assert (exp_reason == 0).any(), kind


# ------------------------------------------------------------------ 8. refusals and marks
def check_refusals_and_marks(v):
    lib, ctx = v.lib, v.ctx
    msgs = list(encoded(3, "finality", "deneb"))
    buf = np.frombuffer(b"".join(msgs), np.uint8)
    lens = np.array([len(m) for m in msgs], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    status = np.full(3, 0xEE, np.uint8)
    codes = np.zeros(3, np.uint8)
    h = C.c_void_p(1)

    def call(**kw):
        a = dict(ctx=ctx, buf=ptr(buf), buf_len=buf.size, offsets=ptr(offs, C.c_uint64), lengths=ptr(lens, C.c_uint64),
                 n=3, kind=1, fork=0, forks=None, status=ptr(status), out=C.byref(h))
        a.update(kw)
        h.value = 1
        rc = lib.lcv_batch_decode(*a.values())
        if a["out"] is not None and a["ctx"] is not None:
            assert rc != -1 or not h.value          # *out = NULL on a refusal
        return rc, lib.lcv_last_error(ctx).decode()

    for name in ("buf", "offsets", "lengths", "status", "out"):
        rc, err = call(**{name: None})
        assert rc == -1 and "null" in err, name
    assert lib.lcv_batch_decode(None, ptr(buf), buf.size, ptr(offs, C.c_uint64), ptr(lens, C.c_uint64), 3, 1, 0, None,
                                ptr(status), C.byref(h)) == -1
    for kind in (3, -1):
        rc, err = call(kind=kind)
        assert rc == -1 and "kind" in err
    for fork in (3, -1):
        rc, err = call(fork=fork)
        assert rc == -1 and "fork" in err
    rc, err = call(fork=3, forks=ptr(codes))  # (ignored with a per-message list)
    assert rc == 0 and h.value
    lib.lcv_batch_free(ctx, h)
    status[:] = 0xEE
    big = np.zeros(65537, np.uint64)
    rc, err = call(n=65537, offsets=ptr(big, C.c_uint64), lengths=ptr(big, C.c_uint64))
    assert rc == -1 and "LCV_DECODE_MAX_ROWS" in err
    for o, ln in ((int(offs[2]), int(lens[2]) + 1), (buf.size, 1), (2 ** 64 - 1, 2), (1, 2 ** 64 - 1), (2 ** 63, 2 ** 63)):
        o3, l3 = offs.copy(), lens.copy()
        o3[2], l3[2] = o, ln
        rc, err = call(offsets=ptr(o3, C.c_uint64), lengths=ptr(l3, C.c_uint64))
        assert rc == -1 and "message 2" in err and "buf_len" in err, (o, ln, err)
    # staged bytes: 65536 entries naming the same 32 KiB window are staged 65536 times (2 GiB and the padding)
    win = np.zeros(32768, np.uint8)
    many_o, many_l = np.zeros(65536, np.uint64), np.full(65536, 32768, np.uint64)
    st2 = np.full(65536, 0xEE, np.uint8)
    rc, err = call(buf=ptr(win), buf_len=win.size, n=65536, offsets=ptr(many_o, C.c_uint64), lengths=ptr(many_l, C.c_uint64),
                   status=ptr(st2))
    assert rc == -1 and "LCV_DECODE_MAX_BYTES" in err and "message 65535" in err and (st2 == 0xEE).all()
    assert (status == 0xEE).all()
    # no message
    rc, err = call(n=0)
    assert rc == 0 and not h.value and (status == 0xEE).all()
    rb, ok = v.decode_resident([], "update")
    assert rb.n == 0 and ok.shape == (0,) and v.download(rb).n == 0
    # the marks: the public stage list has not grown, and a decode leaves no public timing
    assert lib.lcv_stage_name(22) == b"wire_encode" and lib.lcv_stage_name(23) == b"?" and lib.lcv_stage_name(24) == b"?"
    rb, ok = v.decode_resident(msgs, "finality")
    rb.free()
    t = v.last_timings()
    assert len(t) == 23 and all(x == 0.0 for x in t.values()), t
    assert v.last_decode_timings()[0] > 0
    n_out = C.c_uint64()
    assert lib.lcv_batch_shape(ctx, None, C.byref(n_out), C.byref(n_out)) == -1
