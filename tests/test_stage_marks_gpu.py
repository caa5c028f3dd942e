"""GPU: the stage marks Verifier.last_timings reports per call shape on the device (HIP event pairs around the
stages' kernels) — the names bench.py's per-kernel roofline reads.  Cases: tests/stage_mark_cases.py, a few rows
each; the sliced pipeline takes the 300 rows it needs to slice."""
import pytest

import stage_mark_cases as M

pytestmark = pytest.mark.gpu


def test_one_update_fan_engine(gpu_verifier):
    M.check_one_update(gpu_verifier)


def test_six_rows_batch_engine(gpu_verifier):
    M.check_six_rows_batch_engine(gpu_verifier)


@pytest.mark.parametrize("latency_rows", [64, 0])
def test_fold(gpu_verifier, latency_rows):
    M.check_fold(gpu_verifier, latency_rows)


@pytest.mark.parametrize("latency_rows", [64, 0])
def test_dedup(gpu_verifier, latency_rows):
    M.check_dedup(gpu_verifier, latency_rows)


def test_sliced_pipeline(gpu_verifier):
    M.check_sliced_pipeline(gpu_verifier)


def test_setup(gpu_verifier):
    M.check_setup(gpu_verifier)
