"""CPU (host simulation): the stage marks Verifier.last_timings reports per call shape — the names bench.py's
per-kernel roofline reads.  Cases: tests/stage_mark_cases.py; the device runs the same in
tests/test_stage_marks_gpu.py."""
import pytest

import stage_mark_cases as M


def test_one_update_fan_engine(sim_verifier):
    M.check_one_update(sim_verifier)


def test_six_rows_batch_engine(sim_verifier):
    M.check_six_rows_batch_engine(sim_verifier)


@pytest.mark.parametrize("latency_rows", [64, 0])
def test_fold(sim_verifier, latency_rows):
    M.check_fold(sim_verifier, latency_rows)


@pytest.mark.parametrize("latency_rows", [64, 0])
def test_dedup(sim_verifier, latency_rows):
    M.check_dedup(sim_verifier, latency_rows)


def test_sliced_pipeline(sim_verifier):
    M.check_sliced_pipeline(sim_verifier)


def test_setup(sim_verifier):
    M.check_setup(sim_verifier)
