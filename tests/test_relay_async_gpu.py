"""MI355X: the asynchronous relay (lcv_relay_async, lcv_slot_wait_relay; the F_wire_relay kernel of liblcv.so) against
the host decoder, the synchronous relay and the store-table validation: the checks of relay_async_cases.py, which
test_relay_async_hostsim.py runs on the host simulation of the same code."""
import pytest

import relay_async_cases as RA

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", RA.KINDS)
def test_fixture_parity_gpu(gpu_verifier, kind):
    RA.check_fixture(gpu_verifier, kind)


@pytest.mark.parametrize("kind", RA.KINDS)
def test_forks_gpu(gpu_verifier, kind):
    RA.check_forks(gpu_verifier, kind)


@pytest.mark.parametrize("nmsg,nstore", RA.SHAPES)
def test_shapes_gpu(gpu_verifier, nmsg, nstore):
    RA.check_shape(gpu_verifier, nmsg, nstore)


def test_fan_rows_gpu(gpu_verifier):
    RA.check_fan_rows(gpu_verifier)


@pytest.mark.parametrize("n", RA.PAIRS)
def test_npairs_gpu(gpu_verifier, n):
    RA.check_npairs(gpu_verifier, n)


def test_classes_gpu(gpu_verifier):
    RA.check_classes(gpu_verifier)


def test_golden_messages_gpu(gpu_verifier):
    RA.check_golden(gpu_verifier)


def test_malformed_gpu(gpu_verifier):
    RA.check_malformed(gpu_verifier)


def test_status_of_an_unnamed_message_gpu(gpu_verifier):
    RA.check_unnamed_status(gpu_verifier)


def test_eight_in_flight_gpu(gpu_verifier):
    RA.check_slots(gpu_verifier)


def test_mixed_traffic_gpu(gpu_verifier):
    RA.check_mixed_traffic(gpu_verifier)


def test_fold_gpu(gpu_verifier):
    RA.check_fold(gpu_verifier)


def test_rlc_gpu(gpu_verifier):
    RA.check_rlc(gpu_verifier)


def test_refusals_gpu(gpu_verifier):
    v = gpu_verifier
    fresh = type(v)(v.device, lib=v.lib)  # a context with no table and no relay
    try:
        RA.check_refusals(v, fresh)
    finally:
        fresh.close()


@pytest.mark.parametrize("in_flight", [1, 3, 8])
def test_relay_stream_gpu(gpu_verifier, in_flight):
    RA.check_stream(gpu_verifier, in_flight)
