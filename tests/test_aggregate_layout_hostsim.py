"""CPU: the 4-lane masked aggregation (item_agg_team, host-simulation build) on participant sets placed by its
layout — quarters, tree rounds, the complement step — against sums of the oracle's points (tests/aggregate_cases.py)."""
import pytest

import aggregate_cases as A


def test_sets_mean_what_they_say():
    A.layout().check_relations()


@pytest.mark.parametrize("n", A.CALL_SIZES)
def test_aggregate_layout_hostsim(sim_verifier, n):
    A.check_call(sim_verifier, n)
