"""GPU: one call validates a store-table batch and folds it per store (F_fold_seg of csrc/lcv_k_fold.hip behind the
verdicts, one team per store present) — the cases of tests/store_fold_multi_cases.py, which
tests/test_store_fold_multi_hostsim.py runs on the host simulation."""
import pytest

import store_fold_multi_cases as SM

pytestmark = pytest.mark.gpu


# ---- the kernel alone
@pytest.mark.no_sop
@pytest.mark.parametrize("name", SM.kernel_case_names())
def test_fold_stores_kernel(gpu_verifier, name):
    SM.check_kernel_case(gpu_verifier, name)


# ---- end to end, both engines (the fan engine takes batches of at most 64 rows: its calls are cut at 64)
def fan_chunk(v):
    return 64 if v.latency_mode else None


def test_multi_reproduces_fold_sequence(engine_verifier):
    stats = []
    SM.check_multi_sequence(engine_verifier, stats=stats, chunk=fan_chunk(engine_verifier))
    assert all(s["rounds"] >= 3 for s in stats), stats


def test_multi_reproduces_fold_sequence_from_objects(engine_verifier):
    SM.check_multi_sequence(engine_verifier, from_packed=False, chunk=fan_chunk(engine_verifier))


def test_multi_under_pipeline(engine_verifier):
    v = engine_verifier
    prev = v.pipeline
    v.set_pipeline(2, 2)
    try:
        SM.check_multi_sequence(v, chunk=fan_chunk(v))
    finally:
        v.set_pipeline(*prev)


def test_multi_carries_states_between_chunks(engine_verifier):
    SM.check_chunk_carry(engine_verifier)


def test_multi_stores_with_different_committees(engine_verifier):
    SM.check_different_committees(engine_verifier)


def test_async_one_store_and_table_fold_in_flight(engine_verifier):
    SM.check_async(engine_verifier)


@pytest.mark.no_sop
def test_refusals(gpu_verifier):
    from lcv.device import Verifier
    SM.check_refusals(gpu_verifier, lambda: Verifier(0, lib=gpu_verifier.lib))  # a second context: no table set
