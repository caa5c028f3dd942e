"""CPU: the per-update decision of the device code (host-simulation build) at slot, period, fork and participation
boundaries — the fixture tests/golden/lc_boundaries.npz, whose expected reasons come from exec'ing the reference's
own validate_light_client_update under the fixture's small configuration (tests/boundary_cases.py)."""
import pytest

import boundary_cases as BC


def _differences(fx, got, exp):
    return [(fx["names"][i], int(got[i]), int(exp[i])) for i in range(BC.ncases(fx)) if int(got[i]) != int(exp[i])]


def test_fixture_coverage():
    BC.check_coverage(BC.load())


@pytest.mark.slow
def test_oracle_agrees_with_fixture():
    """oracle/sync_protocol.py re-judges every case under the fixture's configuration."""
    fx = BC.load()
    assert not _differences(fx, BC.oracle_reasons(fx, fx["cfg"]), fx["expected_reason"])


def test_single_store_hostsim(sim_verifier):
    fx = BC.load()
    assert not _differences(fx, BC.run_single_store(sim_verifier, fx), fx["expected_reason"])


def test_store_table_hostsim(sim_verifier):
    """item_pre_table and item_nsc_eq_team: every case against its own row of a store table."""
    fx = BC.load()
    got, calls, same = BC.run_store_table(sim_verifier, fx)
    assert not _differences(fx, got, fx["expected_reason"])
    # few calls, and neighbouring rows on different stores (all but a few: one store holds a fifth of the cases)
    assert calls < BC.ncases(fx) // 4 and same <= BC.ncases(fx) // 10


def test_resident_hostsim(sim_verifier):
    got, exp = BC.run_resident(sim_verifier, BC.load())
    assert got.tolist() == exp.tolist()


def test_mainnet_configuration_hostsim(sim_verifier):
    """The same rows under mainnet (32 slots per epoch: every small slot is before Altair and in period 0) against
    the oracle under mainnet: the device reads the configuration, not constants."""
    from lcv.config import MAINNET
    fx = BC.load()
    exp = BC.oracle_reasons(fx, MAINNET)
    assert exp != fx["expected_reason"].tolist()
    assert sum(1 for a, b in zip(exp, fx["expected_reason"]) if a != int(b)) >= BC.ncases(fx) // 4
    assert not _differences(fx, BC.run_single_store(sim_verifier, fx, cfg=MAINNET), exp)
    assert sim_verifier.config == MAINNET
