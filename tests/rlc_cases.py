"""Shared cases of the batch-verification tests (tests/test_rlc_hostsim.py on the host simulation, tests/test_rlc_gpu.py
on the device): with Verifier.set_rlc(G, seed) a group of G consecutive items of a batch-engine chunk pays one final
exponentiation over the product of the items' randomly scaled Miller values, and only the items of a failing group one
of their own (include/lcv.h "Batch verification").

The yardstick of every case is the same call with the mode off: verdict and reason bytes must be exactly equal, no
tolerance, and Verifier.last_rlc must report the groups and the retried rows the case was built with.  Rows come from
the store-table tests' updates (store_table_cases: A and B signed by committee c0, C by c1), so nothing new is signed.
A fixed seed, group 4 and set_latency_mode(0) — the batch engine — unless a case says otherwise."""
import contextlib
import hashlib

import numpy as np

import dedup_cases as D
import store_table_cases as T

LCV_EINVAL = -1
SEED = bytes(range(1, 33))
GROUP = 4
pair, same, edit, latency, base = D.pair, D.same, D.edit, D.latency, D.base


# ------------------------------------------------------------------ plumbing
@contextlib.contextmanager
def rlc(v, group=GROUP, seed=SEED):
    """set_rlc(group, seed) for the block; the verifier is shared by the session, so off again afterwards."""
    v.set_rlc(group, seed)
    try:
        yield
    finally:
        v.set_rlc(0)


def check(v, call, groups, retried, slot=0, group=GROUP, latency_rows=0):
    """The call with the mode off, then on: equal verdicts and reasons, last_rlc == (0, 0) off and (groups, retried)
    on.  Returns (reasons, engine log of the call with the mode on)."""
    with latency(v, latency_rows):
        off = call()
        assert v.last_rlc(slot) == (0, 0)
        with rlc(v, group):
            v.engine_log(reset=True)
            on = call()
            log = v.engine_log(reset=True)
            got = v.last_rlc(slot)
    assert same(off, on), (pair(off)[1].tolist(), pair(on)[1].tolist())
    ok, reason = pair(on)
    assert np.array_equal(ok, reason == 0)
    assert got == (groups, got[1] if retried is None else retried), got
    return reason.tolist(), log


def validate(v, case, p):
    return lambda: v.validate(p, case["current_slot"], case["gvr"])


def nine(v):
    """Nine valid rows A B A B ... : two full groups of four and a tail of one."""
    case, upd = base(v)
    return case, edit(T.take(upd, [0, 1, 0, 1, 0, 1, 0, 1, 0]), sync_signature=1, finality_branch=1)


# ------------------------------------------------------------------ 1, 2, 5: valid rows, wrong signatures
def run_all_valid(v):
    case, p = nine(v)
    return check(v, validate(v, case, p), 3, 0)


def run_one_wrong(v, row):
    """Row `row` (an A) carries B's signature -> reasons; the retried rows are asserted by the caller's numbers."""
    case, p = nine(v)
    assert row % 2 == 0
    p.sync_signature[row] = np.frombuffer(D.wrong_key_signature(v), np.uint8)
    return case, p


def run_every_row_bad(v):
    case, upd = base(v)
    p = edit(T.take(upd, [0] * 8), sync_signature=1)
    p.sync_signature[:] = np.frombuffer(D.wrong_key_signature(v), np.uint8)
    return check(v, validate(v, case, p), 2, 8)[0]


# ------------------------------------------------------------------ 3: a pair that cancels without randomisation
def run_cancelling_pair(v):
    """Rows [A', B', A, B] with S_A' = S_A + D and S_B' = S_B - D: the product of the four UNSCALED pairing values is 1,
    so only distinct coefficients make the group fail -> (reasons, the coefficients of items 0 and 1 for the first
    batch counters)."""
    from oracle import bls12_381 as B
    case, upd = base(v)
    p = edit(T.take(upd, [0, 1, 0, 1]), sync_signature=1)
    d = B.g2_mul(B.G2_GEN, 0x1234567)
    sa = B.g2_decompress(p.sync_signature[0].tobytes())
    sb = B.g2_decompress(p.sync_signature[1].tobytes())
    p.sync_signature[0] = np.frombuffer(B.g2_compress(B.g2_add(sa, d)), np.uint8)
    p.sync_signature[1] = np.frombuffer(B.g2_compress(B.g2_add(sb, B.g2_neg(d))), np.uint8)
    reasons, _ = check(v, validate(v, case, p), 1, 4)
    with rlc(v):
        coeffs = [v.debug_rlc_coeffs(c, 2).tolist() for c in range(16)]
    return reasons, coeffs


# ------------------------------------------------------------------ 4: excluded rows
def run_excluded(v):
    """One group: a signature outside G2, an undecodable signature, a corrupted finality branch (reason 10), one valid
    row.  The three are excluded from the product, which then passes: nothing is retried."""
    case, upd = base(v)
    p = edit(T.take(upd, [0, 0, 0, 0]), sync_signature=1, finality_branch=1)
    p.sync_signature[0] = np.frombuffer(D.non_subgroup_signature(), np.uint8)
    p.sync_signature[1, 0] &= 0x7F  # the compression flag cleared: no valid encoding
    p.finality_branch[2, 7] ^= 0x10
    return check(v, validate(v, case, p), 1, 0)[0]


# ------------------------------------------------------------------ 6: chunks and the other entries
def run_chunks(v):
    """The nine rows under 5-row chunks (5 + 4: groups 2 + 1), one wrong signature in the second chunk."""
    import store_serving_cases as SV
    case, p = run_one_wrong(v, 6)
    with SV.chunk(v, 5):
        return check(v, validate(v, case, p), 3, 4)[0]


def run_store_table(v):
    """validate_stores (the store-table entry) over the semantics rows of the store-table tests."""
    import store_serving_cases as SV
    case, p, index = SV.sem_batch(v)
    T.set_table(v, case)
    n = p.n
    reasons, _ = check(v, lambda: v.validate_stores(p, index, case["current_slot"], case["gvr"]), (n + GROUP - 1) // GROUP,
                       None)
    return reasons


def run_fold(v):
    """validate_fold over five rows (one wrong signature): verdicts and the fold's result equal the mode off."""
    from dataclasses import asdict
    from lcv.device import FoldState
    case, upd = base(v)
    p = edit(T.take(upd, [0, 1, 0, 1, 0]), sync_signature=1)
    p.sync_signature[2] = np.frombuffer(D.wrong_key_signature(v), np.uint8)
    cs, gvr = case["current_slot"], case["gvr"]
    with latency(v, 0):
        off = v.validate_fold(p, cs, gvr, FoldState())
        with rlc(v):
            on = v.validate_fold(p, cs, gvr, FoldState())
            got = v.last_rlc()
    assert same(off, on) and asdict(off[2]) == asdict(on[2])
    assert got == (2, 4), got
    return pair(on)[1].tolist()


def run_async(v):
    """validate_async on slot 3 and the resident entries: results and last_rlc(slot) as the synchronous call's."""
    case, p = run_one_wrong(v, 2)
    cs, gvr = case["current_slot"], case["gvr"]
    with latency(v, 0):
        want = pair(v.validate(p, cs, gvr))
        with rlc(v):
            v.validate_async(p, cs, gvr, 3)
            got = v.slot_wait(3, p.n)
            assert same(got, want) and v.last_rlc(3) == (3, 4), v.last_rlc(3)
            rb = v.upload(p)
            try:
                assert same(v.validate_resident(rb, cs, gvr), want) and v.last_rlc() == (3, 4)
                v.validate_resident_async(rb, cs, gvr, 5)
                assert same(v.slot_wait(5, p.n), want) and v.last_rlc(5) == (3, 4)
            finally:
                rb.free()
    return want[1].tolist()


# ------------------------------------------------------------------ 7: with dedup
def run_with_dedup(v):
    """dedup_cases.basic_rows (6 rows, 3 items) with both modes on, group 2: groups over the 3 items (2), the failing
    item's group retried."""
    case, p = D.basic_rows(v)
    call = validate(v, case, p)
    with latency(v, 0):
        off = call()
        with D.dedup(v, True), rlc(v, 2):
            on = call()
            dd, rl = v.last_dedup(), v.last_rlc()
    assert same(off, on), (pair(off)[1].tolist(), pair(on)[1].tolist())
    return pair(on)[1].tolist(), dd, rl


# ------------------------------------------------------------------ 8: fan engine
def run_fan(v):
    case, p = nine(v)
    return check(v, validate(v, case, p), 0, 0, latency_rows=64)


# ------------------------------------------------------------------ 9: refusals, mode off
def run_refusals(v):
    from lcv._native import LcvError
    import pytest
    bad = pytest.raises(LcvError, match=f"status {LCV_EINVAL}")
    try:
        for g in (1, 3, 5, 6, 12, 128, 65):
            with bad:
                v.set_rlc(g, SEED)
            assert v.rlc_group == 0
        with bad:
            v.set_rlc(4, bytes(32))
        v.set_rlc(4, SEED)
        with bad:
            v.set_pipeline(2, 2)
        assert v.pipeline == (1, 1)
        v.set_pipeline(1, 4)  # one stream: no slicing
        v.set_pipeline(1, 1)
        v.set_rlc(0)
        v.set_pipeline(2, 2)
        with bad:
            v.set_rlc(4, SEED)
        assert v.rlc_group == 0
        v.set_rlc(0)  # off is always accepted
    finally:
        v.set_pipeline(1, 1)
        v.set_rlc(0)


def stages(v):
    return sorted(k for k, ms in v.last_timings().items() if ms > 0)


def run_mode_off(v, fresh):
    """`fresh`: a context of v's backend that never heard of the mode.  The engine log and the stages of the 9-row call
    there on both engines, and of the same calls after the mode was on and off again -> (before, after)."""
    case, p = nine(v)
    c = T.committees(v)
    fresh.set_store(case["stores"][0][0], c[0].ssz, c[1].ssz)
    call = validate(fresh, case, p)

    def observe():
        out = []
        for rows in (0, 64):
            with latency(fresh, rows):
                fresh.engine_log(reset=True)
                res = pair(call())
                out.append((fresh.engine_log(reset=True), stages(fresh), fresh.last_rlc(), res[1].tolist()))
        return out

    before = observe()
    with latency(fresh, 0), rlc(fresh):
        call()
        assert fresh.last_rlc() == (3, 0) and "rlc_scale" in stages(fresh) and "rlc_product" in stages(fresh)
    return before, observe()


# ------------------------------------------------------------------ 10, 11: the hooks
def coeffs_expected(counter, n, seed=SEED):
    out = []
    for i in range(n):
        h = hashlib.sha256(seed + counter.to_bytes(8, "little") + i.to_bytes(4, "little")).digest()
        out.append(int.from_bytes(h[:8], "little") or 1)
    return out


def run_coeffs(v):
    with rlc(v):
        return [(v.debug_rlc_coeffs(c, 70).tolist(), coeffs_expected(c, 70)) for c in (0, 1)]


def run_scale(v):
    """r P from the scaling kernel against the oracle's g1_mul -> (got, want) as lists of 96-byte rows."""
    from oracle import bls12_381 as B
    c = T.committees(v)
    rng = np.random.default_rng(2025)
    rs = [1, 2, 3, 1 << 32, 1 << 63, (1 << 64) - 1] + [int(x) for x in rng.integers(1, 1 << 63, 5, dtype=np.uint64) * 2 + 1]
    pts = [B.G1_GEN, B.g1_neg(B.G1_GEN), B.g1_decompress(bytes(c[0].ssz[:48])), B.g1_decompress(bytes(c[1].ssz[48 * 7:48 * 8]))]
    enc = lambda q: q[0].to_bytes(48, "big") + q[1].to_bytes(48, "big")  # noqa: E731
    rows = [(q, r) for q in pts for r in rs]
    p96 = np.frombuffer(b"".join(enc(q) for q, _ in rows), np.uint8).reshape(-1, 96)
    got = v.debug_rlc_scale(p96, np.array([r for _, r in rows], np.uint64))
    want = [enc(B.g1_mul(q, r)) for q, r in rows]
    return [g.tobytes() for g in got], want
