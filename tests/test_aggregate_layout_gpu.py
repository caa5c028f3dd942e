"""GPU: F_agg_team on the MI355X on participant sets placed by its layout — quarters, tree rounds, the complement
step, item counts around the 16 teams of a wave — against sums of the oracle's points (tests/aggregate_cases.py).

LCV_TEST_HOSTSIM=1 runs the same tests on the host simulation of the device code (CPU dry run)."""
import pytest

import aggregate_cases as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", A.CALL_SIZES)
def test_aggregate_layout_gpu(gpu_verifier, n):
    A.check_call(gpu_verifier, n)
