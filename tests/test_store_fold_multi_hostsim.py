"""CPU (host simulation of the same functors): one call validates a store-table batch and folds it per store — the
segmented fold kernel alone against a sequential model per store, lcv.store.fold_light_client_updates_multi on the
committed sequence and on stores with different committees, the asynchronous entries, the refusals.  Cases:
tests/store_fold_multi_cases.py; the device runs the same in tests/test_store_fold_multi_gpu.py."""
import pytest

import helpers as H
import store_fold_multi_cases as SM


@pytest.mark.parametrize("name", SM.kernel_case_names())
def test_fold_stores_kernel(sim_verifier, name):
    SM.check_kernel_case(sim_verifier, name)


def test_multi_reproduces_fold_sequence(sim_verifier):
    SM.check_multi_sequence(sim_verifier)


def test_multi_reproduces_fold_sequence_in_chunks(sim_verifier):
    SM.check_multi_sequence(sim_verifier, from_packed=False, chunk=64)


def test_multi_carries_states_between_chunks(sim_verifier):
    SM.check_chunk_carry(sim_verifier)


def test_multi_stores_with_different_committees(sim_verifier):
    SM.check_different_committees(sim_verifier)


def test_async_one_store_and_table_fold_in_flight(sim_verifier):
    SM.check_async(sim_verifier)


def test_refusals(sim_verifier):
    SM.check_refusals(sim_verifier, H.hostsim_verifier)
