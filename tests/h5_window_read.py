"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.read_frames with rows / cols
against the slices of the whole read.  Prints 'OK' lines; tests/test_window_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ebcc_amd import h5_batch  # noqa: E402

out = sys.argv[1]
H, W = 200, 300
rng = np.random.default_rng(11)
y, x = np.mgrid[0:H, 0:W]
data = np.stack([(280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32)
                 for k in range(10)]).reshape(2, 5, H, W)
data[1, 2] = -4.25                                               # constant field
opt = ("max_error_target", 0.05)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


with h5py.File(os.path.join(out, "w.h5"), "w") as f:
    d = h5_batch.create_dataset(f, "t", data.shape, 20, opt)
    h5_batch.write_frames(d, data, 20, opt)
with h5py.File(os.path.join(out, "w.h5"), "r") as f:
    whole = h5_batch.read_frames(f["t"])
    via_callback = f["t"][...]
    assert whole.shape == data.shape and np.array_equal(bits(whole), bits(via_callback))
    assert np.array_equal(bits(h5_batch.read_frames(f["t"], rows=None, cols=None)), bits(whole))
    assert np.array_equal(bits(h5_batch.read_frames(f["t"], rows=slice(None), cols=slice(0, W))), bits(whole))
    print("OK defaults and whole-frame slices give the whole read")
    for rows, cols in [(slice(60, 127), slice(101, 230)), (slice(0, 1), None), (None, slice(W - 1, W)), (slice(-40, None), slice(-33, -1)),
                       (slice(63, 65), slice(127, 129)), (slice(5, 190), slice(7, 9))]:
        got = h5_batch.read_frames(f["t"], rows=rows, cols=cols, batch=4)
        want = whole[..., rows if rows is not None else slice(None), cols if cols is not None else slice(None)]
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(bits(got), bits(want)), (rows, cols)
    print("OK read_frames(rows, cols) == read_frames()[..., rows, cols]")
    for rows, cols in [(slice(10, 10), None), (None, slice(0, W, 2)), (slice(H, H + 5), None), (3, None)]:
        try:
            h5_batch.read_frames(f["t"], rows=rows, cols=cols)
        except (ValueError, TypeError):
            continue
        raise AssertionError(f"accepted rows={rows} cols={cols}")
    print("OK empty, strided and non-slice selections are refused")
