"""CPU: the device SSZ encoder (lcv_batch_encode, lcv_encode_updates; csrc/lcv_wire_enc.hpp) on the host simulation
of the kernel's code, against the reference-serialised messages and lcv.wire.encode_updates.  The same checks run on
the MI355X in test_wire_encode_gpu.py; both live in wire_encode_cases.py."""
import pytest

import wire_encode_cases as WE


def test_generator_rows_encodable_and_cover_every_residue():
    WE.check_generator()


def test_fork_digests():
    WE.check_fork_digests()


def test_reference_bytes(sim_verifier):
    WE.check_reference_bytes(sim_verifier)


@pytest.mark.parametrize("fork", WE.FORKS)
@pytest.mark.parametrize("kind", WE.KINDS)
def test_differential(sim_verifier, kind, fork):
    WE.check_differential(sim_verifier, kind, fork, 130)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_shapes(sim_verifier, n):
    WE.check_differential(sim_verifier, "update", "deneb", n)
    WE.check_differential(sim_verifier, "finality", "capella", n)


def test_every_byte_written(sim_verifier):
    WE.check_every_byte_written(sim_verifier)


def test_auto_fork(sim_verifier):
    WE.check_auto_fork(sim_verifier)


def test_statuses(sim_verifier):
    WE.check_statuses(sim_verifier)


def test_row_lists_and_chunks(sim_verifier):
    WE.check_rows_and_chunks(sim_verifier)


def test_resident_producer_batch_and_updates_by_range(sim_verifier):
    WE.check_resident_producer(sim_verifier)


def test_refusals_and_stage(sim_verifier):
    WE.check_refusals_and_stage(sim_verifier)
