"""CPU: the batched producer entries (lcv_create_updates*, lcv_create_bootstraps, lcv_batch_download,
lcv_rank_resident) on the host simulation of the kernels' code (lcv_producer.hpp), against the reference's fixture
and against lcv/producer.py's per-object functions.  The same checks run on the MI355X in
test_producer_batch_gpu.py; both live in producer_batch_cases.py."""
import pytest

import producer_batch_cases as PB


def test_generator_covers_every_case():
    PB.check_generator_coverage()


def test_reference_fixture(sim_verifier):
    PB.check_reference_fixture(sim_verifier)


@pytest.mark.parametrize("kind", ["update", "finality", "optimistic"])
def test_differential(sim_verifier, kind):
    PB.check_differential(sim_verifier, kind)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_shapes(sim_verifier, n):
    PB.check_differential(sim_verifier, n=n)


def test_single_view(sim_verifier):
    PB.check_single_view(sim_verifier)


def test_single_committee(sim_verifier):
    PB.check_differential(sim_verifier, ncomm=1)


def test_bootstraps_differential(sim_verifier):
    PB.check_bootstraps_differential(sim_verifier)


def test_resident_batch_validates(sim_verifier):
    PB.check_resident_validates(sim_verifier)


def test_resident_rank_download_best(sim_verifier):
    PB.check_resident_rank_download(sim_verifier)


def test_refusals(sim_verifier):
    PB.check_refusals(sim_verifier)


def test_stage_names_and_timings(sim_verifier):
    PB.check_stage_names(sim_verifier)
