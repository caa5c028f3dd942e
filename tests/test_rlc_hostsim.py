"""CPU: randomised batch verification (Verifier.set_rlc, include/lcv.h "Batch verification") on the host simulation —
the scaling, the signature walk with its own second point, the product tree, the groups' final exponentiation, the
spread and the counted retry as plain loops, through the staged / resident / asynchronous / table / fold entries.
Every case compares verdicts and reasons with the same call with the mode off and asserts last_rlc
(tests/rlc_cases.py)."""
import pytest

import helpers as H
import rlc_cases as R


@pytest.fixture(scope="module")
def v(sim_verifier):
    return sim_verifier


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
    fresh = H.hostsim_verifier()
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


def test_work_check_covers_the_scratch(v):
    fresh = H.hostsim_verifier()
    try:
        assert fresh.lib.lcv_debug_work_check(fresh.ctx, 200, 64, 3) == 0
    finally:
        fresh.close()


def test_cpu_baseline_build_runs_every_row(v):
    """The CPU-baseline library (LCV_CPU_FAST: run_bls's direct branch) accepts the mode, keeps running every row and
    reports 0 groups."""
    import os
    import subprocess
    from lcv._native import Lib
    from lcv.device import Verifier
    path = os.path.join(H.PKG, "build", "liblcv_cpu.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "build/liblcv_cpu.so"], cwd=H.PKG)
    cpu = Verifier(lib=Lib(path))
    try:
        case, p = R.run_one_wrong(v, 4)
        c = R.T.committees(v)
        cpu.set_store(case["stores"][0][0], c[0].ssz, c[1].ssz)
        with R.latency(cpu, 0), R.rlc(cpu):
            ok, reason = cpu.validate(p, case["current_slot"], case["gvr"])
            assert reason.tolist() == [0, 0, 0, 0, 14, 0, 0, 0, 0] and cpu.last_rlc() == (0, 0)
    finally:
        cpu.close()
