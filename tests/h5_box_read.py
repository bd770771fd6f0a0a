"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.read_boxes and read_points against
indexing of the whole read.  Prints 'OK' lines; tests/test_box_decode_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ebcc_amd import h5_batch  # noqa: E402

out = sys.argv[1]
H, W = 100, 130
rng = np.random.default_rng(13)
y, x = np.mgrid[0:H, 0:W]
data = np.stack([(280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32)
                 for k in range(12)]).reshape(3, 4, H, W)
data[1, 2] = -4.25                                               # constant field
opt = ("max_error_target", 0.05)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


with h5py.File(os.path.join(out, "b.h5"), "w") as f:
    d = h5_batch.create_dataset(f, "t", data.shape, 20, opt)
    h5_batch.write_frames(d, data, 20, opt)
with h5py.File(os.path.join(out, "b.h5"), "r") as f:
    whole = h5_batch.read_frames(f["t"])
    assert whole.shape == data.shape and np.array_equal(bits(whole), bits(f["t"][...]))
    flat = whole.reshape(-1, H, W)
    for rows, cols, k, batch in [(17, 29, 40, 5), (1, 1, 64, 256), (H, W, 5, 2), (32, 32, 9, 3)]:
        boxes = np.stack([rng.integers(0, 12, k), rng.integers(0, H - rows + 1, k), rng.integers(0, W - cols + 1, k)], axis=1)     # (frames in any order)
        if k == 9:
            boxes[:, 0] = [6, 6, 6, 2, 2, 9, 9, 9, 9]                                                                          # few frames named
        got = h5_batch.read_boxes(f["t"], boxes, rows, cols, batch=batch)
        want = np.stack([flat[fr, r0:r0 + rows, c0:c0 + cols] for fr, r0, c0 in boxes])
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (rows, cols)
    print("OK read_boxes == read_frames().reshape(-1, H, W)[frame, row0:row0 + rows, col0:col0 + cols]")
    for k in (1, 7, 64):
        ri, ci = rng.integers(0, H, k), rng.integers(0, W, k)
        ri[0], ci[0] = H - 1, W - 1
        got = h5_batch.read_points(f["t"], ri, ci, batch=5)
        want = whole[..., ri, ci]
        assert got.shape == (3, 4, k) == want.shape and np.array_equal(bits(got), bits(want)), k
    assert np.array_equal(bits(h5_batch.read_points(f["t"], [-1, 0], [-1, 5])), bits(whole[..., [-1, 0], [-1, 5]]))
    print("OK read_points == read_frames()[..., rows_idx, cols_idx]")
    for bad in [np.array([[12, 0, 0]]), np.array([[0, H - 16, 0]]), np.array([[0, 0, W - 28]]), np.array([[-1, 0, 0]]), np.zeros((0, 3), np.int64)]:
        try:
            h5_batch.read_boxes(f["t"], bad, 17, 29)
        except ValueError:
            continue
        raise AssertionError(f"accepted boxes {bad.tolist()}")
    try:
        h5_batch.read_points(f["t"], [H], [0])
    except IndexError:
        pass
    else:
        raise AssertionError("accepted a point outside the frame")
    print("OK boxes outside the frames and points outside the frame are refused")
