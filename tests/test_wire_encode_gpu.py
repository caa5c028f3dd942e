"""MI355X: the device SSZ encoder (lcv_batch_encode, lcv_encode_updates; the F_wire_enc kernel of liblcv.so) against
the reference-serialised messages and lcv.wire.encode_updates: the checks of wire_encode_cases.py, which
test_wire_encode_hostsim.py runs on the host simulation of the same code."""
import pytest

import wire_encode_cases as WE

pytestmark = pytest.mark.gpu


def test_reference_bytes_gpu(gpu_verifier):
    WE.check_reference_bytes(gpu_verifier)


@pytest.mark.parametrize("fork", WE.FORKS)
@pytest.mark.parametrize("kind", WE.KINDS)
def test_differential_gpu(gpu_verifier, kind, fork):
    WE.check_differential(gpu_verifier, kind, fork, 130)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_shapes_gpu(gpu_verifier, n):
    WE.check_differential(gpu_verifier, "update", "deneb", n)
    WE.check_differential(gpu_verifier, "finality", "capella", n)


def test_every_byte_written_gpu(gpu_verifier):
    WE.check_every_byte_written(gpu_verifier)


def test_auto_fork_gpu(gpu_verifier):
    WE.check_auto_fork(gpu_verifier)


def test_statuses_gpu(gpu_verifier):
    WE.check_statuses(gpu_verifier)


def test_row_lists_and_chunks_gpu(gpu_verifier):
    WE.check_rows_and_chunks(gpu_verifier)


def test_resident_producer_batch_and_updates_by_range_gpu(gpu_verifier):
    WE.check_resident_producer(gpu_verifier)


def test_refusals_and_stage_gpu(gpu_verifier):
    WE.check_refusals_and_stage(gpu_verifier)
