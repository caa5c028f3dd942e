"""GPU: what each wait returns for each way a batch was put on a work-space slot, cell by cell, on both engines — the
cases of tests/slot_wait_cases.py, which tests/test_slot_wait_hostsim.py runs on the host simulation."""
import pytest

import slot_wait_cases as SW

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("entry", SW.ENTRIES)
def test_every_wait_after(engine_verifier, entry):
    SW.check_entry(engine_verifier, entry)


def test_more_rows_than_the_batch(engine_verifier):
    SW.check_more_rows_than_the_batch(engine_verifier)


def test_slot_reused_by_another_kind(engine_verifier):
    SW.check_reuse_by_another_kind(engine_verifier)
