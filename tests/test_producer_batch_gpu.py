"""MI355X: the batched producer entries on the device — the cases of test_producer_batch_hostsim.py
(producer_batch_cases.py) through liblcv.so's kernels (lcv_k_prod.hip)."""
import pytest

import producer_batch_cases as PB

pytestmark = pytest.mark.gpu


def test_reference_fixture_gpu(gpu_verifier):
    PB.check_reference_fixture(gpu_verifier)


@pytest.mark.parametrize("kind", ["update", "finality", "optimistic"])
def test_differential_gpu(gpu_verifier, kind):
    PB.check_differential(gpu_verifier, kind)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_shapes_gpu(gpu_verifier, n):
    PB.check_differential(gpu_verifier, n=n)


def test_single_view_gpu(gpu_verifier):
    PB.check_single_view(gpu_verifier)


def test_single_committee_gpu(gpu_verifier):
    PB.check_differential(gpu_verifier, ncomm=1)


def test_bootstraps_differential_gpu(gpu_verifier):
    PB.check_bootstraps_differential(gpu_verifier)


def test_resident_batch_validates_gpu(engine_verifier):
    PB.check_resident_validates(engine_verifier)


def test_resident_rank_download_best_gpu(gpu_verifier):
    PB.check_resident_rank_download(gpu_verifier)


def test_refusals_gpu(gpu_verifier):
    PB.check_refusals(gpu_verifier)


def test_stage_names_and_timings_gpu(gpu_verifier):
    PB.check_stage_names(gpu_verifier)
