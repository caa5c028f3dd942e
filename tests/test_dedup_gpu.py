"""GPU: the deduplicated BLS half (Verifier.set_dedup, include/lcv.h "Deduplicated signatures") on the device —
F_dedup_gather and F_verdict_dedup around the unchanged BLS kernels on both engines, the two-stream ordering behind
the gather, the staged / resident / asynchronous / fold shapes.  Every case compares verdicts and reasons with the
same call under set_dedup(False) and asserts last_dedup (tests/dedup_cases.py); a few rows each."""
import pytest

import dedup_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def v(gpu_verifier):
    return gpu_verifier


def test_basic_merge_fan_engine(v):
    reasons, log = D.run_basic(v, 64)
    assert reasons == D.BASIC_REASONS
    assert log["fan"] > 0 and log["twin"] > 0 and log["batch"] == 0 and log["lane"] == 0, log


def test_basic_merge_batch_engine(v):
    reasons, log = D.run_basic(v, 0)
    assert reasons == D.BASIC_REASONS
    assert log["batch"] > 0 and log["lane"] > 0 and log["fan"] == 0 and log["twin"] == 0, log


def test_shared_item_different_pre_checks(v):
    assert D.run_shared_item(v) == [0, 10, 1]


def test_shared_failing_item_wrong_key(v):
    assert D.run_shared_failure(v, D.wrong_key_signature(v)) == [14] * 4


def test_shared_failing_item_outside_g2(v):
    assert D.run_shared_failure(v, D.non_subgroup_signature()) == [14] * 4


def test_store_table(v):
    assert D.run_table(v, duplicate_row=False) == [0, 0, 0, 14]


def test_store_table_duplicate_committee_row(v):
    reasons = D.run_table(v, duplicate_row=True)  # (2 items asserted inside: the equal rows are not merged)
    assert reasons == [0, 0, 0, 0]


def test_golden_replay(v):
    got, want, items, cases = D.run_golden(v)
    assert got.tolist() == want.tolist()
    assert items <= cases


def test_collisions_basic(v):
    reasons, _ = D.run_basic(v, 64, hash_bits=0)
    assert reasons == D.BASIC_REASONS


def test_collisions_store_table(v):
    assert D.run_table(v, duplicate_row=False, hash_bits=0) == [0, 0, 0, 14]
    assert D.run_table(v, duplicate_row=True, hash_bits=0) == [0, 0, 0, 0]


def test_engine_by_items(v):
    got, want, log, d = D.run_engine_by_items(v)
    assert got.tolist() == want.tolist() == [0] * 70
    assert d == (70, 2)
    assert log["fan"] > 0 and log["twin"] > 0 and log["batch"] == 0 and log["lane"] == 0, log


def test_chunks(v):
    reasons, d, per_chunk = D.run_chunks(v)
    assert reasons.tolist() == [0] * 130
    assert per_chunk == 3 + 3 + 2 and d == (130, per_chunk)


def test_async_two_slots(v):
    D.run_async(v)


def test_resident(v):
    D.run_resident(v)


def test_fold(v):
    D.run_fold(v)


def test_validate_stream(v):
    D.run_stream(v)


def test_pipeline_refused(v):
    D.run_pipeline_refused(v)


def test_mode_off_launches_unchanged(v):
    fresh = type(v)(v.device, lib=v.lib)  # a context on which the mode was never on
    try:
        before, after = D.run_mode_off(v, fresh)
    finally:
        fresh.close()
    assert before == after and before["fan"] > 0
