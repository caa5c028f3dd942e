"""CPU: the device SSZ decoder (lcv_batch_decode; csrc/lcv_wire_dec.hpp) on the host simulation of the kernels' code,
against the host decoder (csrc/lcv_wire.cpp).  The same checks run on the MI355X in test_wire_decode_gpu.py; both live
in wire_decode_cases.py."""
import pytest

import wire_decode_cases as WD


def test_reference_bytes(sim_verifier):
    WD.check_reference_bytes(sim_verifier)


@pytest.mark.parametrize("fork", WD.FORKS)
@pytest.mark.parametrize("kind", WD.KINDS)
def test_differential(sim_verifier, kind, fork):
    WD.check_differential(sim_verifier, kind, fork, 130)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_shapes(sim_verifier, n):
    WD.check_differential(sim_verifier, "update", "deneb", n)
    WD.check_differential(sim_verifier, "finality", "capella", n)


@pytest.mark.parametrize("kind", WD.KINDS)
def test_mixed_forks(sim_verifier, kind):
    WD.check_mixed_forks(sim_verifier, kind)


@pytest.mark.parametrize("fork", WD.FORKS)
@pytest.mark.parametrize("kind", WD.KINDS)
def test_round_trip(sim_verifier, kind, fork):
    WD.check_round_trip(sim_verifier, kind, fork)


@pytest.mark.parametrize("fork", WD.FORKS)
@pytest.mark.parametrize("kind", WD.KINDS)
def test_malformed(sim_verifier, kind, fork):
    WD.check_malformed(sim_verifier, kind, fork)


@pytest.mark.parametrize("kind", WD.KINDS)
def test_fork_code_out_of_range(sim_verifier, kind):
    WD.check_fork_code_3(sim_verifier, kind)


def test_buffer_forms(sim_verifier):
    WD.check_buffer_forms(sim_verifier)
    WD.check_buffer_forms(sim_verifier, "finality", "capella")


def test_pool(sim_verifier):
    WD.check_pool(sim_verifier)


def test_validate_where_it_lies(sim_verifier):
    WD.check_validate(sim_verifier)


def test_refusals_and_marks(sim_verifier):
    WD.check_refusals_and_marks(sim_verifier)
