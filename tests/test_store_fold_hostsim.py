"""CPU (host simulation of the same functors): the store fold — rank records against the reference's own
is_better_update, the fold kernel alone against a sequential model, lcv.store's fold entries on the committed
sequences.  Cases: tests/store_fold_cases.py; the device runs the same in tests/test_store_fold_gpu.py."""
import pytest

import store_fold_cases as SF


def test_rank_orders_pairs_as_the_reference(sim_verifier):
    SF.check_rank_matrix(sim_verifier)


def test_rank_key_is_the_device_record(sim_verifier):
    SF.check_rank_key(sim_verifier)


def test_best_update_per_period(sim_verifier):
    SF.check_best_per_period(sim_verifier)


def test_unpack_update_inverts_packing():
    SF.check_unpack_roundtrip()


@pytest.mark.parametrize("name", SF.fold_case_names())
def test_fold_kernel(sim_verifier, name):
    SF.check_fold_case(sim_verifier, name)


def test_fold_row_limit(sim_verifier):
    SF.check_fold_limits(sim_verifier)


def test_fold_reproduces_older_sequence(sim_verifier):
    SF.check_store_sequence(sim_verifier)


def test_fold_reproduces_fold_sequence(sim_verifier):
    SF.check_fold_sequence(sim_verifier)


def test_table_batch_refused(sim_verifier):
    SF.check_table_batch_refused(sim_verifier)


def test_async_two_slots(sim_verifier):
    SF.check_async_two_slots(sim_verifier)
