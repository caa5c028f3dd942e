"""CPU: a store per update (lcv_set_store_table + lcv_validate_updates_stores) and the one-call range sync built on
it (lcv.store.sync_light_client_updates), on the host simulation of the device code.  Yardsticks: the single-store
path (lcv_set_store + lcv_validate_updates once per distinct store), the reference-exec'd goldens, and
process_light_client_updates.  Inputs and runners: tests/store_table_cases.py."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import store_cases
import store_table_cases as T

LCV_EINVAL, LCV_ESTATE = -1, -4


@pytest.fixture(scope="module")
def v():
    return H.hostsim_verifier()


def test_goldens_in_fewer_calls(v):
    """Every lc_updates golden case, grouped by current_slot only: the cases' stores are rows of one table."""
    got, exp, calls = T.run_golden_cases(v)
    assert list(got) == list(exp)
    assert calls < 13  # the single-store runner (golden_cases.run_update_cases) needs one call per (store, slot): 13


def test_per_row_semantics(v):
    got, want = T.run_semantics(v)
    assert list(got) == list(want)
    assert list(got) == T.SEM_EXPECTED


def test_index_checks():
    """Every index is checked on the host: the refused calls launch nothing (no work space exists afterwards, and
    the engine log counts no launch)."""
    from lcv._native import StoreTable, ptr
    v = H.hostsim_verifier()
    case_p = T.take(_tiny_batch(), [0])
    b, keep = case_p.to_c()
    gvr = np.zeros(32, np.uint8)
    out = np.zeros(2, np.uint8)

    def validate(index):
        ix = np.asarray(index, np.uint32)
        return v.lib.lcv_validate_updates_stores(v.ctx, C.byref(b), ptr(ix, C.c_uint32), 1, ptr(gvr), ptr(out), ptr(out[1:]))

    def set_table(ncomm, cur, nxt, rows=None):
        com = np.zeros((ncomm if rows is None else rows, T.SC_BYTES), np.uint8)
        fin = np.zeros(len(cur), np.uint64)
        cur, nxt = np.asarray(cur, np.uint32), np.asarray(nxt, np.uint32)
        t = StoreTable(ptr(com), ncomm, ptr(fin, C.c_uint64), ptr(cur, C.c_uint32), ptr(nxt, C.c_uint32), len(cur))
        return v.lib.lcv_set_store_table(v.ctx, C.byref(t), None)

    assert validate([0]) == LCV_ESTATE
    assert b"lcv_set_store_table" in v.lib.lcv_last_error(v.ctx)
    assert set_table(2, [0, 2], [1, 1]) == LCV_EINVAL           # current == ncomm
    assert b"current[1]" in v.lib.lcv_last_error(v.ctx)
    assert set_table(2, [0, 1, 0], [1, T.UNKNOWN, 2]) == LCV_EINVAL   # next == ncomm (the sentinel before it is fine)
    assert b"next[2]" in v.lib.lcv_last_error(v.ctx)
    assert set_table(4097, [0], [T.UNKNOWN], rows=1) == LCV_EINVAL     # ncomm above LCV_STORE_TABLE_MAX_COMMITTEES
    assert b"ncomm" in v.lib.lcv_last_error(v.ctx)
    assert validate([0]) == LCV_ESTATE  # none of them set a table
    # a table of 2 stores over one (all-zero) committee, then store_index == nstore
    assert set_table(1, [0, 0], [T.UNKNOWN, 0]) == 0
    v.engine_log(reset=True)
    assert validate([2]) == LCV_EINVAL
    assert b"store_index[0]" in v.lib.lcv_last_error(v.ctx)
    log = v.engine_log()
    assert (log["fan"], log["batch"], log["twin"], log["lane"]) == (0, 0, 0, 0)


def _tiny_batch():
    from lcv.device import PackedUpdates
    z = lambda w: np.zeros((1, w), np.uint8)  # noqa: E731
    return PackedUpdates(att_beacon=z(112), att_exec=z(832), att_branch=z(128), fin_beacon=z(112), fin_exec=z(832),
                         fin_branch=z(128), nsc_pool=z(T.SC_BYTES), nsc_index=np.zeros(1, np.uint32), nsc_branch=z(160),
                         finality_branch=z(192), sync_bits=z(64), sync_signature=z(96),
                         signature_slot=np.zeros(1, np.uint64))


def test_chunk_offset(v):
    got, want = T.run_chunks(v)
    assert list(got) == list(want)


def _same(old, new):
    assert new["accepted"] == old["accepted"]
    assert new["reasons"] == old["reasons"]
    assert new["summary"] == old["summary"]


def test_range_sync_three_periods(v):
    old, new = T.run_sync(v, T.chain_case(v))
    _same(old, new)
    assert all(old["accepted"]) and len(old["accepted"]) == 6
    assert new["stats"]["validate_calls"] == 1 and new["validations"] == 1
    assert new["stats"]["rows_validated"] == 6
    assert old["validations"] >= 3


def test_range_sync_with_a_bad_row(v):
    case = T.chain_case(v, bad_first_of_second_period=True)
    old, new = T.run_sync(v, case)
    _same(old, new)
    assert old["reasons"][2] == 14 and not old["accepted"][2]
    assert 1 < new["stats"]["validate_calls"] <= old["validations"]
    # the good chain with an update repeated
    ups = T.chain_case(v)["updates"]
    old, new = T.run_sync(v, T.chain_case(v), ups[:3] + [ups[2]] + ups[3:])
    _same(old, new)
    assert new["stats"]["validate_calls"] <= old["validations"]


def test_existing_sequence(v):
    """The reference-exec'd store sequence (tests/golden/store_sequence.npz), both next_known cases."""
    from lcv import store as LS
    z, p = store_cases.load()
    n = len(z["kinds"])
    cur, nxt = z["current_committee"].tobytes(), z["next_committee"].tobytes()
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    for case, next_known in enumerate((1, 0)):
        ups = [H.update_from(p, i) for i in range(n)]
        st = H.store_from(int(z["store_finalized_slot"]), cur, nxt if next_known else bytes(24624))
        reasons, stats = [], {}
        acc = LS.sync_light_client_updates(st, ups, cs, gvr, v, reasons, stats)
        assert list(acc.astype(np.uint8)) == list(z["accepted"][case])
        assert reasons == list(z["reason"][case])
        assert store_cases.summary(st) == list(z["summary"][case][n - 1])
        assert stats["rows_validated"] >= n and stats["validate_calls"] >= 1
