"""CPU: the asynchronous relay (lcv_relay_async, lcv_slot_wait_relay; F_wire_relay of csrc/lcv_wire_dec.hpp) on the host
simulation of the kernels' code.  The same checks run on the MI355X in test_relay_async_gpu.py; both live in
relay_async_cases.py."""
import pytest

import helpers as H
import relay_async_cases as RA


@pytest.mark.parametrize("kind", RA.KINDS)
def test_fixture_parity(sim_verifier, kind):
    RA.check_fixture(sim_verifier, kind)


@pytest.mark.parametrize("kind", RA.KINDS)
def test_forks(sim_verifier, kind):
    RA.check_forks(sim_verifier, kind)


@pytest.mark.parametrize("nmsg,nstore", RA.SHAPES)
def test_shapes(sim_verifier, nmsg, nstore):
    RA.check_shape(sim_verifier, nmsg, nstore)


def test_fan_rows(sim_verifier):
    RA.check_fan_rows(sim_verifier)


@pytest.mark.parametrize("n", RA.PAIRS)
def test_npairs(sim_verifier, n):
    RA.check_npairs(sim_verifier, n)


def test_classes(sim_verifier):
    RA.check_classes(sim_verifier)


def test_golden_messages(sim_verifier):
    RA.check_golden(sim_verifier)


def test_malformed(sim_verifier):
    RA.check_malformed(sim_verifier)


def test_status_of_an_unnamed_message(sim_verifier):
    RA.check_unnamed_status(sim_verifier)


def test_eight_in_flight(sim_verifier):
    RA.check_slots(sim_verifier)


def test_mixed_traffic(sim_verifier):
    RA.check_mixed_traffic(sim_verifier)


def test_fold(sim_verifier):
    RA.check_fold(sim_verifier)


def test_rlc(sim_verifier):
    RA.check_rlc(sim_verifier)


def test_refusals(sim_verifier):
    RA.check_refusals(sim_verifier, H.hostsim_verifier())


@pytest.mark.parametrize("in_flight", [1, 3, 8])
def test_relay_stream(sim_verifier, in_flight):
    RA.check_stream(sim_verifier, in_flight)
