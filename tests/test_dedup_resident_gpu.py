"""GPU: classes of a resident batch made where it lies (Verifier.classify_resident: F_dedup_key and F_dedup_confirm,
16-lane teams, the host's grouping between them), Verifier.fan_out (F_prod_pick into a table batch) and
lcv.serving.relay_updates on the device.  Cases and yardsticks: tests/dedup_resident_cases.py; at most 281 rows each."""
import pytest

import dedup_resident_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def v(gpu_verifier):
    return gpu_verifier


@pytest.mark.parametrize("n", R.SIZES)
def test_classes_equal_the_hosts(v, n):
    R.check_sizes(v, n)


def test_classes_across_chunks(v):
    R.check_sizes(v, 130, chunk=64)


def test_every_tuple_byte_counts(v):
    R.check_flip_table(v)


def test_non_tuple_columns_do_not_count(v):
    R.check_non_tuple_columns(v)


def test_collisions(v):
    R.check_collisions(v)


@pytest.mark.parametrize("latency_rows", [64, 0])
def test_verdicts_decoded(v, latency_rows):
    R.check_verdicts_decoded(v, latency_rows)


@pytest.mark.parametrize("latency_rows", [64, 0])
def test_verdicts_created(v, latency_rows):
    R.check_verdicts_created(v, latency_rows)


def test_fan_out_rows(v):
    R.check_fan_out(v)


def test_relay(v):
    R.check_relay(v)


def test_refusals(v):
    R.check_refusals(v)


def test_existing_behaviour(v):
    R.check_existing_behaviour(v)
