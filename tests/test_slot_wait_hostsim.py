"""CPU (host simulation of the same driver): what each wait returns for each way a batch was put on a work-space slot,
cell by cell — the cases of tests/slot_wait_cases.py; the device runs the same in tests/test_slot_wait_gpu.py."""
import pytest

import slot_wait_cases as SW


@pytest.mark.parametrize("entry", SW.ENTRIES)
def test_every_wait_after(sim_verifier, entry):
    SW.check_entry(sim_verifier, entry)


def test_more_rows_than_the_batch(sim_verifier):
    SW.check_more_rows_than_the_batch(sim_verifier)


def test_slot_reused_by_another_kind(sim_verifier):
    SW.check_reuse_by_another_kind(sim_verifier)
