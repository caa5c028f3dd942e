"""GPU: a store per update (lcv_set_store_table + lcv_validate_updates_stores: the per-row pre-check kernel and the
per-row committee-equality team kernel) and the one-call range sync on liblcv.so, on the fan engine and on the batch
engine.  The same cases as tests/test_store_table_hostsim.py (tests/store_table_cases.py), against the single-store
path on the same device and the reference-exec'd goldens."""
import pytest

import helpers as H
import store_table_cases as T

pytestmark = pytest.mark.gpu


def test_goldens_in_fewer_calls_gpu(engine_verifier):
    got, exp, _ = T.run_golden_cases(engine_verifier)
    assert list(got) == list(exp)


def test_per_row_semantics_gpu(engine_verifier):
    got, want = T.run_semantics(engine_verifier)
    assert list(got) == list(want)
    assert list(got) == T.SEM_EXPECTED


def test_chunk_offset_gpu(engine_verifier):
    got, want = T.run_chunks(engine_verifier)
    assert list(got) == list(want)


def test_range_sync_three_periods_gpu(engine_verifier):
    old, new = T.run_sync(engine_verifier, T.chain_case(engine_verifier))
    assert new["accepted"] == old["accepted"] and all(old["accepted"])
    assert new["reasons"] == old["reasons"]
    assert new["summary"] == old["summary"]
    assert new["stats"]["validate_calls"] == 1 and new["validations"] == 1
    assert old["validations"] >= 3


def test_multi_store_objects_gpu(engine_verifier):
    """The 10-row batch of the semantics test through validate_light_client_updates_multi with store OBJECTS: repeated
    objects and equal stores held by different objects land on one table row, and an unchanged table is not
    uploaded again."""
    from lcv.sync_protocol import validate_light_client_updates_multi
    case = T.semantics_case(engine_verifier)
    p = T.take(case["updates"], [u for u, _ in case["rows"]])
    want = T.yardstick(engine_verifier, p, [T.store_key(case, s) for _, s in case["rows"]], case["current_slot"],
                       case["gvr"])
    shared = {s: H.store_from(*T.store_key(case, s)) for s in range(len(case["stores"]))}
    cv = T.CountingVerifier(engine_verifier)
    for fresh in (False, True):  # one object per distinct store, then one object per row
        stores = [H.store_from(*T.store_key(case, s)) if fresh else shared[s] for _, s in case["rows"]]
        ok, got = validate_light_client_updates_multi(stores, p, case["current_slot"], case["gvr"], cv)
        assert list(got) == list(want)
        assert list(ok) == [r == 0 for r in want]
    assert cv.uploads == 1 and cv.validations == 2
