"""GPU: the store fold on the device (F_rank, F_fold of csrc/lcv_k_fold.hip behind the verdicts) — the cases of
tests/store_fold_cases.py, which tests/test_store_fold_hostsim.py runs on the host simulation."""
import numpy as np
import pytest

import store_cases
import store_fold_cases as SF

pytestmark = pytest.mark.gpu


# ---- rank parity
@pytest.mark.no_sop
def test_rank_orders_pairs_as_the_reference(engine_verifier):
    SF.check_rank_matrix(engine_verifier)


@pytest.mark.no_sop
def test_rank_key_is_the_device_record(engine_verifier):
    SF.check_rank_key(engine_verifier)


@pytest.mark.no_sop
def test_best_update_per_period(engine_verifier):
    SF.check_best_per_period(engine_verifier)


# ---- the fold kernel alone
@pytest.mark.no_sop
@pytest.mark.parametrize("name", SF.fold_case_names())
def test_fold_kernel(gpu_verifier, name):
    SF.check_fold_case(gpu_verifier, name)


@pytest.mark.no_sop
def test_fold_row_limit(gpu_verifier):
    SF.check_fold_limits(gpu_verifier)


# ---- end to end, both engines
def test_fold_reproduces_older_sequence(engine_verifier):
    SF.check_store_sequence(engine_verifier)


def test_fold_reproduces_fold_sequence(engine_verifier):
    stats = []
    SF.check_fold_sequence(engine_verifier, stats=stats)
    assert all(s["segments"] >= 3 for s in stats), stats  # two applying rows and what follows them


def test_fold_reproduces_fold_sequence_from_objects(engine_verifier):
    SF.check_fold_sequence(engine_verifier, from_packed=False)


def test_fold_every_prefix(engine_verifier):
    f = SF.fixture()
    SF.check_every_prefix(engine_verifier, SF.sequence_rows(), f["seq_summary"], f["seq_accepted"])


def test_fold_equals_process_light_client_updates(engine_verifier):
    SF.check_equals_sibling(engine_verifier, SF.sequence_rows())


def test_fold_under_pipeline(engine_verifier):
    v = engine_verifier
    prev = v.pipeline
    v.set_pipeline(2, 2)
    try:
        SF.check_fold_sequence(v)
    finally:
        v.set_pipeline(*prev)


def test_fold_under_pipeline_sliced(gpu_verifier):
    """Enough rows for lcv_set_pipeline(2, 2) to cut slices (>= 256): the fold runs after all slices have joined.
    320 sub-2/3 rows, every fifth invalid, then an applying row; against process_light_client_updates."""
    _, p = store_cases.load()
    rows = SF.take(p, [0, 1, 4, 8, 3] * 64 + [11, 0])
    v = gpu_verifier
    prev = v.pipeline
    v.set_pipeline(2, 2)
    try:
        SF.check_equals_sibling(v, rows)
    finally:
        v.set_pipeline(*prev)


def test_async_two_slots(engine_verifier):
    SF.check_async_two_slots(engine_verifier)


@pytest.mark.no_sop
def test_table_batch_refused(gpu_verifier):
    SF.check_table_batch_refused(gpu_verifier)
