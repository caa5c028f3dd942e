"""CPU, no library: PackedUpdates' check(), empty(), slice() and to_c() against its one column table (_SPEC)."""
import ctypes as C
from dataclasses import fields

import numpy as np
import pytest

from lcv import layout as L
from lcv.device import PackedUpdates

N, NPOOL = 5, 2
COLUMNS = list(PackedUpdates._SPEC)
# what include/lcv.h says of lcv_update_batch, written out independently of _SPEC
WANT = dict(att_beacon=(np.uint8, (N, 112)), att_exec=(np.uint8, (N, 832)), att_branch=(np.uint8, (N, 128)),
            fin_beacon=(np.uint8, (N, 112)), fin_exec=(np.uint8, (N, 832)), fin_branch=(np.uint8, (N, 128)),
            nsc_pool=(np.uint8, (NPOOL, 24624)), nsc_index=(np.uint32, (N,)), nsc_branch=(np.uint8, (N, 160)),
            finality_branch=(np.uint8, (N, 192)), sync_bits=(np.uint8, (N, 64)), sync_signature=(np.uint8, (N, 96)),
            signature_slot=(np.uint64, (N,)))


def test_spec_is_the_dataclass_and_the_abi():
    assert COLUMNS == [f.name for f in fields(PackedUpdates)] == list(WANT)
    assert L.SYNC_COMMITTEE_BYTES == 24624


def test_empty_has_the_spec_shapes_and_passes_check():
    p = PackedUpdates.empty(N, NPOOL)
    p.check()
    assert p.n == N
    for name, (dt, shape) in WANT.items():
        a = getattr(p, name)
        assert a.dtype == dt and a.shape == shape and a.flags.c_contiguous and not a.any(), name
    PackedUpdates.empty(0, 1).check()


def _double(a, axis):
    """An array twice as long along `axis`, whose every other element is a non-contiguous view of a's shape."""
    big = np.zeros(tuple(2 * s if k == axis else s for k, s in enumerate(a.shape)), a.dtype)
    return big[::2] if axis == 0 else big[:, ::2]


@pytest.mark.parametrize("name", COLUMNS)
def test_check_names_the_offending_column(name):
    dt, shape = WANT[name]

    def refused(a):
        p = PackedUpdates.empty(N, NPOOL)
        setattr(p, name, a)
        with pytest.raises(ValueError, match=f"^{name}: need C-contiguous "):
            p.check()
        with pytest.raises(ValueError, match=f"^{name}: "):
            p.to_c()

    # a wrong trailing width (a 1-D column: a trailing axis it must not have)
    refused(np.zeros(shape[:1] + ((shape[1] + 1,) if len(shape) == 2 else (1,)), dt))
    # a wrong dtype of the same item size, and of another
    refused(np.zeros(shape, np.int8 if dt == np.uint8 else np.int32 if dt == np.uint32 else np.int64))
    refused(np.zeros(shape, np.uint16))
    # a non-contiguous view of the right dtype and shape, along each axis
    for axis in range(len(shape)):
        view = _double(np.zeros(shape, dt), axis)
        assert view.shape == shape and view.dtype == dt and not view.flags.c_contiguous
        refused(view)
    if name not in ("att_beacon", "nsc_pool"):  # (att_beacon's rows define n; the pool's define npool)
        refused(np.zeros((N + 1,) + shape[1:], dt))


def test_check_refuses_an_index_outside_the_pool():
    p = PackedUpdates.empty(N, NPOOL)
    p.nsc_index[3] = NPOOL
    with pytest.raises(ValueError, match="^nsc_index out of range$"):
        p.check()


def test_slice_keeps_the_pool_and_cuts_the_rest():
    p = PackedUpdates.empty(N, NPOOL)
    for name in COLUMNS:
        a = getattr(p, name)
        a.reshape(a.shape[0], -1)[...] = np.arange(a.shape[0])[:, None] + 1
    p.nsc_index[:] = 0
    s = p.slice(1, 4)
    s.check()
    assert s.n == 3 and s.nsc_pool is p.nsc_pool
    for name in COLUMNS:
        if name != "nsc_pool":
            assert np.array_equal(getattr(s, name), getattr(p, name)[1:4]), name
    assert p.slice(2, 2).n == 0


def test_to_c_passes_the_arrays_themselves():
    p = PackedUpdates.empty(N, NPOOL)
    b, keep = p.to_c()
    got = [b.attested.beacon, b.attested.execution, b.attested.exec_branch, b.finalized.beacon, b.finalized.execution,
           b.finalized.exec_branch, b.nsc_pool, b.nsc_index, b.nsc_branch, b.finality_branch, b.sync_bits,
           b.sync_signature, b.signature_slot]
    for name, q in zip(COLUMNS, got):
        assert C.cast(q, C.c_void_p).value == getattr(p, name).ctypes.data, name
    assert (b.n, b.npool) == (N, NPOOL)
    assert all(any(k is getattr(p, name) for k in keep) for name in COLUMNS)
