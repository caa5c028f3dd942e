"""GPU: randomised batch verification (Verifier.set_rlc, include/lcv.h "Batch verification") on the device —
F_rlc_scale, F_sop_lines_g1, the f12mul product tree, the groups' final exponentiation, F_rlc_spread and the counted
retry (k_sop_counted) around the unchanged BLS kernels, with the two-stream ordering behind the scaling.  Every case
compares verdicts and reasons with the same call with the mode off and asserts last_rlc (tests/rlc_cases.py); a
handful of rows each."""
import pytest

import rlc_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def v(gpu_verifier):
    return gpu_verifier


def test_all_valid(v):
    reasons, log = R.run_all_valid(v)
    assert reasons == [0] * 9
    assert log["batch"] > 0 and log["lane"] > 0 and log["fan"] == 0 and log["twin"] == 0, log


def test_one_wrong_signature_middle_group(v):
    case, p = R.run_one_wrong(v, 4)
    reasons, _ = R.check(v, R.validate(v, case, p), 3, 4)
    assert reasons == [0, 0, 0, 0, 14, 0, 0, 0, 0]


def test_one_wrong_signature_tail_group(v):
    case, p = R.run_one_wrong(v, 8)
    reasons, _ = R.check(v, R.validate(v, case, p), 3, 1)
    assert reasons == [0] * 8 + [14]


def test_cancelling_pair(v):
    reasons, coeffs = R.run_cancelling_pair(v)
    assert reasons == [14, 14, 0, 0]
    assert all(c[0] != c[1] for c in coeffs)


def test_excluded_rows_do_not_poison_a_group(v):
    assert R.run_excluded(v) == [14, 14, 10, 0]


def test_every_row_bad(v):
    assert R.run_every_row_bad(v) == [14] * 8


def test_chunks(v):
    assert R.run_chunks(v) == [0, 0, 0, 0, 0, 0, 14, 0, 0]


def test_store_table_entry(v):
    assert R.run_store_table(v) == R.T.SEM_EXPECTED


def test_fold_entry(v):
    assert R.run_fold(v) == [0, 0, 14, 0, 0]


def test_async_and_resident_entries(v):
    assert R.run_async(v) == [0, 0, 14, 0, 0, 0, 0, 0, 0]


def test_with_dedup(v):
    reasons, dd, rl = R.run_with_dedup(v)
    assert reasons == R.D.BASIC_REASONS
    assert dd == (6, 3)
    assert rl[0] == 2 and rl[1] <= 1  # the failing item alone in the tail group: retried, or excluded if undecodable


def test_fan_engine_untouched(v):
    reasons, log = R.run_fan(v)
    assert reasons == [0] * 9
    assert log["fan"] > 0 and log["twin"] > 0 and log["batch"] == 0 and log["lane"] == 0, log


def test_refusals(v):
    R.run_refusals(v)


def test_mode_off_launches_unchanged(v):
    fresh = type(v)(v.device, lib=v.lib)  # a context that never heard of the mode
    try:
        before, after = R.run_mode_off(v, fresh)
    finally:
        fresh.close()
    assert before == after
    assert before[0][0]["batch"] > 0 and before[1][0]["fan"] > 0


def test_coefficients(v):
    for got, want in R.run_coeffs(v):
        assert got == want and all(got)


def test_scaling(v):
    got, want = R.run_scale(v)
    assert got == want
