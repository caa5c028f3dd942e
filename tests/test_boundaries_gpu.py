"""GPU: liblcv.so on the MI355X at slot, period, fork and participation boundaries — the fixture
tests/golden/lc_boundaries.npz (reference-exec'd expected reasons) through the single-store, store-table and
resident paths, on both engines (tests/boundary_cases.py).

LCV_TEST_HOSTSIM=1 runs the same tests on the host simulation of the device code (CPU dry run)."""
import pytest

import boundary_cases as BC

pytestmark = pytest.mark.gpu


def _differences(fx, got, exp):
    return [(fx["names"][i], int(got[i]), int(exp[i])) for i in range(BC.ncases(fx)) if int(got[i]) != int(exp[i])]


def test_single_store_gpu(engine_verifier):
    fx = BC.load()
    BC.check_coverage(fx)
    assert not _differences(fx, BC.run_single_store(engine_verifier, fx), fx["expected_reason"])


def test_store_table_gpu(engine_verifier):
    fx = BC.load()
    got, calls, same = BC.run_store_table(engine_verifier, fx)
    assert not _differences(fx, got, fx["expected_reason"])
    assert same <= BC.ncases(fx) // 10


def test_resident_gpu(engine_verifier):
    got, exp = BC.run_resident(engine_verifier, BC.load())
    assert got.tolist() == exp.tolist()
