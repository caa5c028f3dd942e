"""Shared by test_batch_roundtrip_hostsim.py and test_batch_roundtrip_gpu.py: a host batch whose every byte names
its place goes to the device (lcv_batch_upload, lcv_batch_upload_stores) and comes back (lcv_batch_download, whole
and by rows), so a column that the driver's column table swaps, shifts or sizes wrongly cannot round-trip.  No
validation runs: the only kernel is the row gather of a download by rows."""
import numpy as np

from lcv.device import PackedUpdates

N, NPOOL = 5, 2  # the smallest batch with an interior row between two picked ones and a row picked twice
ROWS = [4, 0, 4]
NSC_INDEX = [1, 0, 1, 1, 0]    # (the upload refuses an index outside the pool, so this column cannot carry the code)
STORE_INDEX = [2, 0, 1, 0, 2]  # (no store table is needed to upload)


def coded_batch() -> PackedUpdates:
    """Byte `off` of row `row` of column `col` is a code of (col, row, off): distinct between neighbouring columns,
    rows and offsets, and not periodic in any power of two."""
    p = PackedUpdates.empty(N, NPOOL)
    for col, name in enumerate(PackedUpdates._SPEC):
        a = getattr(p, name)
        flat = a.view(np.uint8).reshape(a.shape[0], -1)
        row, off = np.indices(flat.shape)
        flat[...] = (73 * (col + 1) + 151 * row + 7 * off + 29 * (off // 251)) % 251
    p.nsc_index[:] = NSC_INDEX
    p.check()
    return p


def assert_columns_equal(got: PackedUpdates, want: PackedUpdates, rows=None):
    for name, (_, _, pool) in PackedUpdates._SPEC.items():
        w = getattr(want, name)
        if rows is not None and not pool:
            w = w[rows]
        g = getattr(got, name)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), name


def check_roundtrip(v, store_index=None):
    p = coded_batch()
    rb = v.upload(p, store_index=store_index)
    try:
        assert_columns_equal(v.download(rb), p)
        assert_columns_equal(v.download(rb, rows=ROWS), p, rows=ROWS)
    finally:
        rb.free()
    assert_columns_equal(p, coded_batch())  # the host batch was only read
