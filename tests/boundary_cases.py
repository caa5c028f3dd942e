"""Shared runner of the boundary fixture (tests/golden/lc_boundaries.npz + .json, made by make_boundary_golden.py),
used by test_boundaries_hostsim.py (host simulation of the kernels' code) and test_boundaries_gpu.py (the MI355X).

The fixture places validate_light_client_update's decision (item_pre_body, lc_header_valid, signing_root and the
masked aggregation) on the slots where it changes its answer: fork epochs' first and last slots, period edges,
current_slot == signature_slot, signature_slot == attested + 1, attested == store finalized + 1, slots around 2^63
and the participation counts around the aggregation's complement threshold — under the small configuration of
producer_batch_cases.small_config() (8 slots per epoch, 8 epochs per period; Altair 8, Bellatrix 16, Capella 24,
Deneb 40; periods from 64 and 128).  Every expected reason is the failing assert of the reference's exec'd
validate_light_client_update; everything here is exact integers: equality, no tolerance.

Layout: each distinct signed row is stored once (the packed columns of include/lcv.h and its signature_slot); a case
is (row, store finalized slot, next committee known, current_slot, pool row).  The committees are rows 0 and 1 of
lc_updates.npz's nsc_pool (row 2: all zero); the store of every case holds row 0 as current and row 1 as next.
"""
import json
import os

import numpy as np

import golden_cases as G
import producer_batch_cases as PB

COLS = G.COLS
UNKNOWN = 0xFFFFFFFF
FAMILIES = ("V", "H", "S", "P", "R", "G", "N")

_cache = {}


def config_from(meta):
    from lcv.config import NetworkConfig
    c = meta["config"]
    return NetworkConfig(**{k: (bytes.fromhex(v) if isinstance(v, str) and k != "name" else v) for k, v in c.items()})


def load():
    """The fixture: its arrays, `names` / `families` per case, `cfg` (the NetworkConfig it was made under) and `pool`."""
    if "fx" not in _cache:
        fx = dict(np.load(os.path.join(G.GOLDEN, "lc_boundaries.npz"), allow_pickle=False))
        meta = json.load(open(os.path.join(G.GOLDEN, "lc_boundaries.json")))
        fx["names"] = [c["name"] for c in meta["cases"]]
        fx["families"] = [c["family"] for c in meta["cases"]]
        fx["cfg"] = config_from(meta)
        fx["pool"] = G.load_updates()["nsc_pool"]
        assert meta["expected_reason"] == fx["expected_reason"].tolist()
        assert fx["cfg"] == PB.small_config()
        _cache["fx"] = fx
    return _cache["fx"]


def ncases(fx):
    return len(fx["case_row"])


def batch(fx, cases):
    """Cases `cases` as a PackedUpdates: each case's row with the case's pool row."""
    from lcv.device import PackedUpdates
    rows = fx["case_row"][list(cases)].astype(np.int64)
    return PackedUpdates(nsc_pool=fx["pool"], nsc_index=fx["case_pool_row"][list(cases)].astype(np.uint32),
                         signature_slot=fx["signature_slot"][rows].copy(),
                         **{k: np.ascontiguousarray(fx[k][rows]) for k in COLS})


def store_of(fx, i):
    return int(fx["case_store_finalized_slot"][i]), int(fx["case_next_known"][i])


def check_coverage(fx):
    """The generator's coverage conditions, on what is loaded: every reason, both verdicts in every family, at
    least 40 % valid and at least 40 % invalid."""
    exp = [int(r) for r in fx["expected_reason"]]
    n = len(exp)
    assert n == ncases(fx) == len(fx["names"]) == len(fx["families"]) and len(set(fx["names"])) == n
    assert set(exp) == set(range(15)), sorted(set(range(15)) - set(exp))
    assert set(fx["families"]) == set(FAMILIES)
    for f in FAMILIES:
        verdicts = {exp[i] == 0 for i in range(n) if fx["families"][i] == f}
        assert verdicts == {True, False}, (f, verdicts)
    valid = sum(1 for r in exp if r == 0)
    assert 5 * valid >= 2 * n and 5 * (n - valid) >= 2 * n, (valid, n)
    # the edges themselves: slots at and above 2^63, every fork epoch's first and last slot as attested slot
    att = {int.from_bytes(fx["att_beacon"][r, :8].tobytes(), "little") for r in fx["case_row"]}
    assert {7, 8, 15, 16, 23, 24, 39, 40, 63, 64, (1 << 63) - 1, (1 << 63) + 1} <= att
    assert int(fx["case_current_slot"].max()) == (1 << 64) - 1 and int(fx["signature_slot"].max()) > 1 << 63
    pc = {int(np.unpackbits(fx["sync_bits"][r]).sum()) for r in fx["case_row"]}
    assert {0, 1, 255, 256, 257, 258, 511, 512} <= pc


def _groups(keys):
    """{key: [case indices]} in sorted key order."""
    out = {}
    for i, k in enumerate(keys):
        out.setdefault(k, []).append(i)
    return dict(sorted(out.items()))


def run_single_store(verifier, fx, cfg=None, max_rows=64):
    """set_store + validate, grouped by (store, current_slot) as golden_cases.run_update_cases does (the store is
    set once per distinct store; a group goes in calls of at most max_rows rows, 64 being the most the fan engine
    takes), under the fixture's configuration or `cfg` -> reason codes in case order."""
    n = ncases(fx)
    cur, nxt, zero = (fx["pool"][k].tobytes() for k in range(3))
    gvr = fx["genesis_validators_root"].tobytes()
    out = np.full(n, 255, np.uint8)
    last = None
    with PB.configured(verifier, cfg or fx["cfg"]):
        for (fin, nk, cs), cases in _groups([store_of(fx, i) + (int(fx["case_current_slot"][i]),) for i in range(n)]).items():
            if (fin, nk) != last:
                verifier.set_store(fin, cur, nxt if nk else zero)
                last = (fin, nk)
            for lo in range(0, len(cases), max_rows):
                part = cases[lo:lo + max_rows]
                ok, reason = verifier.validate(batch(fx, part), cs, gvr)
                assert np.array_equal(ok, reason == 0)
                out[part] = reason
    return out


def interleave(cases, key):
    """`cases` reordered so that neighbours differ in key(case) wherever the group allows it: each key's cases are
    spread evenly over the whole order."""
    lists = _groups([key(i) for i in cases]).values()
    spread = sorted(((k + 0.5) / len(x), j, cases[c]) for j, x in enumerate(lists) for k, c in enumerate(x))
    return [c for _, _, c in spread]


def run_store_table(verifier, fx, max_rows=64):
    """set_store_table (one store row per distinct (finalized slot, next known)) + validate_stores, grouped by
    current_slot with neighbouring rows on different stores; a group goes in calls of at most max_rows rows (64: the
    most the fan engine takes) -> (reasons in case order, number of calls, number of neighbouring pairs that share
    a store)."""
    n = ncases(fx)
    gvr = fx["genesis_validators_root"].tobytes()
    stores = sorted({store_of(fx, i) for i in range(n)})
    index = [stores.index(store_of(fx, i)) for i in range(n)]
    out = np.full(n, 255, np.uint8)
    calls = same = 0
    with PB.configured(verifier, fx["cfg"]):
        verifier.set_store_table(fx["pool"][:2], [s[0] for s in stores], [0] * len(stores),
                                 [1 if s[1] else UNKNOWN for s in stores])
        for cs, cases in _groups([int(fx["case_current_slot"][i]) for i in range(n)]).items():
            group = interleave(cases, lambda i: index[i])
            for lo in range(0, len(group), max_rows):
                cases = group[lo:lo + max_rows]
                six = [index[i] for i in cases]
                same += sum(1 for a, b in zip(six, six[1:]) if a == b)
                ok, reason = verifier.validate_stores(batch(fx, cases), six, cs, gvr)
                assert np.array_equal(ok, reason == 0)
                out[cases] = reason
                calls += 1
    return out, calls, same


def run_resident(verifier, fx):
    """upload + validate_resident of the largest (store, current_slot) group -> (reasons, expected reasons)."""
    n = ncases(fx)
    groups = _groups([store_of(fx, i) + (int(fx["case_current_slot"][i]),) for i in range(n)])
    (fin, nk, cs), cases = max(groups.items(), key=lambda kv: len(kv[1]))
    cases = cases[:64]
    assert len(cases) >= 8
    cur, nxt, zero = (fx["pool"][k].tobytes() for k in range(3))
    with PB.configured(verifier, fx["cfg"]):
        verifier.set_store(fin, cur, nxt if nk else zero)
        rb = verifier.upload(batch(fx, cases))
        try:
            ok, reason = verifier.validate_resident(rb, cs, fx["genesis_validators_root"].tobytes())
        finally:
            rb.free()
    assert np.array_equal(ok.astype(bool), reason == 0)
    return reason, fx["expected_reason"][cases]


def oracle_config(cfg):
    """oracle.spec.use_config's keywords for a NetworkConfig."""
    from oracle.spec import _CONFIG_NAMES
    return {k: getattr(cfg, k) for k in _CONFIG_NAMES}


def oracle_reasons(fx, cfg):
    """Every case judged by oracle.sync_protocol.validate_light_client_update under `cfg` (CPU).  FastAggregateVerify
    is a pure function of its arguments and cases share rows, so its results are memoised for the run."""
    import helpers as H
    from oracle import spec as S
    cur, nxt, zero = (fx["pool"][k].tobytes() for k in range(3))
    gvr = fx["genesis_validators_root"].tobytes()
    fav, memo = S.bls.FastAggregateVerify, {}

    def fav_memo(pks, msg, sig):
        key = (tuple(bytes(p) for p in pks), bytes(msg), bytes(sig))
        if key not in memo:
            memo[key] = fav(pks, msg, sig)
        return memo[key]
    out = []
    S.bls.FastAggregateVerify = fav_memo
    try:
        with S.use_config(**oracle_config(cfg)):
            for i in range(ncases(fx)):
                fin, nk = store_of(fx, i)
                store = H.store_from(fin, cur, nxt if nk else zero)
                out.append(H.O.validate_light_client_update(store, H.update_from(batch(fx, [i]), 0),
                                                            int(fx["case_current_slot"][i]), gvr))
    finally:
        del S.bls.FastAggregateVerify  # (the instance attribute: the class's own function shows again)
    return out
