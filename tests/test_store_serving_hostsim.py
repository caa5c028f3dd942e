"""CPU: table batches (a store row per update) in the resident, asynchronous, piped and sharded shapes, and
lcv.serving.validate_stream, on the host simulation of the device code.  Cases and yardsticks:
tests/store_serving_cases.py — the synchronous validate_stores on the same rows and table, and SEM_EXPECTED."""
import numpy as np
import pytest

import helpers as H
import store_serving_cases as S
import store_table_cases as T


@pytest.fixture(scope="module")
def v():
    return H.hostsim_verifier()


def test_resident(v):
    got, dev, want = S.run_resident(v)
    assert S.same(got, want) and list(got[1]) == T.SEM_EXPECTED
    assert list(dev) == [int(r == 0) for r in T.SEM_EXPECTED]


def test_chunks(v):
    res, host, want64, want1 = S.run_chunks(v)
    assert S.same(want64, want1)
    assert S.same(res, want64)
    assert S.same(host, want1)


def test_slots(v):
    before, after = S.run_slots(v)
    assert after == before


def test_pipeline(v):
    (sync1, res1), (sync2, res2) = S.run_pipeline(v)
    assert S.same(res1, sync1)
    assert S.same(sync2, sync1) and S.same(res2, sync1)


def test_table_replaced(v):
    first, again, old, new = S.run_table_replaced(v)
    assert S.same(first, old) and list(first[1]) == T.SEM_EXPECTED
    assert S.same(again, new)


def test_host_checks(v):
    after = S.run_host_checks(v, H.hostsim_verifier())
    assert len(after) == 6 and all(r == T.SEM_EXPECTED for r in after)


def test_sharded_one_rank(v, tmp_path, monkeypatch):
    monkeypatch.setenv("LCV_RENDEZVOUS_DIR", str(tmp_path))
    full, gathered, want = S.run_sharded(v, "store_serving_hostsim")
    assert np.array_equal(full, want[0]) and np.array_equal(gathered, want[0])


def test_sharded_index_follows_the_rows():
    """multi.validate_sharded cuts store_index at the rows' shard bounds on every rank, and the one-row dummy of an
    empty shard carries index 0 (no device: the verifier and the communicator only record)."""
    from lcv import multi
    _, p, index = S.sem_batch(H.hostsim_verifier())
    p3, index3 = T.take(p, [0, 1]), np.array([4, 2], np.uint32)

    class Recorder:
        def upload(self, batch, store_index=None):
            self.rows, self.index = batch, None if store_index is None else np.array(store_index)
            return self

        def free(self):
            pass

    class OneShot:
        def __init__(self, world, rank):
            self.world, self.rank = world, rank

        def validate_sharded(self, rb, current_slot, gvr, per_rank):
            return np.zeros(self.world * per_rank, np.uint8)

    for batch, six, world in ((p, index, 3), (p3, index3, 3)):
        for rank in range(world):
            rec = Recorder()
            multi.validate_sharded(rec, batch, 1, bytes(32), OneShot(world, rank), store_index=six)
            lo, hi = multi.shard_bounds(batch.n, world, rank)
            if hi > lo:
                assert list(rec.index) == list(six[lo:hi]) and rec.rows.n == hi - lo
                assert np.array_equal(rec.rows.sync_signature, batch.sync_signature[lo:hi])
            else:
                assert list(rec.index) == [0] and rec.rows.n == 1
    rec = Recorder()
    multi.validate_sharded(rec, p, 1, bytes(32), OneShot(2, 1))
    assert rec.index is None
    with pytest.raises(ValueError):
        multi.validate_sharded(rec, p, 1, bytes(32), OneShot(2, 1), store_index=index[:9])


@pytest.mark.parametrize("in_flight", [1, 8])
def test_validate_stream(v, in_flight):
    got, want = S.run_stream(v, in_flight)
    assert len(got) == len(want) == 10
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0].dtype == bool and S.same(g, w), k


def test_validate_stream_arguments(v):
    from lcv.serving import validate_stream
    case, p, index = S.sem_batch(v)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            list(validate_stream(v, [p], case["current_slot"], case["gvr"], in_flight=bad))
    with pytest.raises(ValueError):
        list(validate_stream(v, [(p, index[:3])], case["current_slot"], case["gvr"]))
    assert list(validate_stream(v, [], case["current_slot"], case["gvr"])) == []


def test_store_keys_above_one_chunk_go_through_the_stream(v):
    """validate_under_store_keys keeps its results when a PackedUpdates input above one chunk (64 rows here) takes
    the validate_stream route: no synchronous validate_stores call, the same reasons."""
    from lcv.sync_protocol import validate_under_store_keys
    case, p, index = S.tiled(v, 130)
    keys = [T.store_key(case, int(s)) for s in index]
    cv = T.CountingVerifier(v)
    ok1, r1 = validate_under_store_keys(keys, p, case["current_slot"], case["gvr"], cv)
    assert cv.validations == 1
    with S.chunk(v, 64):
        ok2, r2 = validate_under_store_keys(keys, p, case["current_slot"], case["gvr"], cv)
    assert cv.validations == 1  # the second call made no synchronous call
    assert np.array_equal(r2, r1) and np.array_equal(ok2, ok1) and ok2.dtype == bool
