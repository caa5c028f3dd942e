"""MI355X: the device SSZ decoder (lcv_batch_decode; the F_wire_dec, F_sc_confirm and F_sc_gather kernels of
liblcv.so) against the host decoder: the checks of wire_decode_cases.py, which test_wire_decode_hostsim.py runs on the
host simulation of the same code."""
import pytest

import wire_decode_cases as WD

pytestmark = pytest.mark.gpu


def test_reference_bytes_gpu(gpu_verifier):
    WD.check_reference_bytes(gpu_verifier)


@pytest.mark.parametrize("fork", WD.FORKS)
@pytest.mark.parametrize("kind", WD.KINDS)
def test_differential_gpu(gpu_verifier, kind, fork):
    WD.check_differential(gpu_verifier, kind, fork, 130)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_shapes_gpu(gpu_verifier, n):
    WD.check_differential(gpu_verifier, "update", "deneb", n)
    WD.check_differential(gpu_verifier, "finality", "capella", n)


@pytest.mark.parametrize("kind", WD.KINDS)
def test_mixed_forks_gpu(gpu_verifier, kind):
    WD.check_mixed_forks(gpu_verifier, kind)


@pytest.mark.parametrize("fork", WD.FORKS)
@pytest.mark.parametrize("kind", WD.KINDS)
def test_round_trip_gpu(gpu_verifier, kind, fork):
    WD.check_round_trip(gpu_verifier, kind, fork)


@pytest.mark.parametrize("fork", WD.FORKS)
@pytest.mark.parametrize("kind", WD.KINDS)
def test_malformed_gpu(gpu_verifier, kind, fork):
    WD.check_malformed(gpu_verifier, kind, fork)


@pytest.mark.parametrize("kind", WD.KINDS)
def test_fork_code_out_of_range_gpu(gpu_verifier, kind):
    WD.check_fork_code_3(gpu_verifier, kind)


def test_buffer_forms_gpu(gpu_verifier):
    WD.check_buffer_forms(gpu_verifier)
    WD.check_buffer_forms(gpu_verifier, "finality", "capella")


def test_pool_gpu(gpu_verifier):
    WD.check_pool(gpu_verifier)


def test_validate_where_it_lies_gpu(gpu_verifier):
    WD.check_validate(gpu_verifier)


def test_refusals_and_marks_gpu(gpu_verifier):
    WD.check_refusals_and_marks(gpu_verifier)
