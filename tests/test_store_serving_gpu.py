"""GPU: table batches (a store row per update) in the resident, asynchronous, piped and sharded shapes, and
lcv.serving.validate_stream, on liblcv.so.  The same cases as tests/test_store_serving_hostsim.py
(tests/store_serving_cases.py), against the synchronous validate_stores on the same device and SEM_EXPECTED; cases of
at most 64 rows run on the fan engine and on the batch engine."""
import os

import numpy as np
import pytest

import store_serving_cases as S
import store_table_cases as T

pytestmark = pytest.mark.gpu


def test_resident_gpu(engine_verifier):
    got, dev, want = S.run_resident(engine_verifier)
    assert S.same(got, want) and list(got[1]) == T.SEM_EXPECTED
    assert list(dev) == [int(r == 0) for r in T.SEM_EXPECTED]


def test_chunks_gpu(gpu_verifier):
    res, host, want64, want1 = S.run_chunks(gpu_verifier)
    assert S.same(want64, want1)
    assert S.same(res, want64)
    assert S.same(host, want1)


def test_slots_gpu(engine_verifier):
    before, after = S.run_slots(engine_verifier)
    assert after == before


def test_pipeline_gpu(gpu_verifier):
    (sync1, res1), (sync2, res2) = S.run_pipeline(gpu_verifier)
    assert S.same(res1, sync1)
    assert S.same(sync2, sync1) and S.same(res2, sync1)


def test_table_replaced_gpu(engine_verifier):
    first, again, old, new = S.run_table_replaced(engine_verifier)
    assert S.same(first, old) and list(first[1]) == T.SEM_EXPECTED
    assert S.same(again, new)


def test_table_replaced_under_a_long_batch_gpu(gpu_verifier):
    """2,000 rows on the batch engine are still running when set_store_table is called: without the drain, the new
    store columns could land under the batch in flight."""
    first, again, old, new = S.run_table_replaced(gpu_verifier, tiles=200)
    assert S.same(first, old) and S.same(again, new)


def test_host_checks_gpu(engine_verifier):
    if S.is_hostsim(engine_verifier):
        import helpers as H
        fresh = H.hostsim_verifier()
    else:
        from lcv.device import Verifier
        fresh = Verifier(engine_verifier.device)
    try:
        fresh.set_latency_mode(engine_verifier.latency_mode)
        after = S.run_host_checks(engine_verifier, fresh)
    finally:
        fresh.close()
    assert len(after) == 6 and all(r == T.SEM_EXPECTED for r in after)


def test_sharded_one_rank_gpu(engine_verifier):
    full, gathered, want = S.run_sharded(engine_verifier, f"store_serving_{os.getpid()}")
    assert np.array_equal(full, want[0]) and np.array_equal(gathered, want[0])


@pytest.mark.parametrize("in_flight", [1, 8])
def test_validate_stream_gpu(gpu_verifier, in_flight):
    got, want = S.run_stream(gpu_verifier, in_flight)
    assert len(got) == len(want) == 10
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0].dtype == bool and S.same(g, w), k
