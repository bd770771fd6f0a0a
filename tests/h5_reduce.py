"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.reduce_frames against the same
reduction - a loop over the frames in order, in float64 - of h5_batch.read_frames.  Prints 'OK' lines;
tests/test_reduce_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ebcc_amd import h5_batch  # noqa: E402

out = sys.argv[1]
H, W = 64, 96
SCALES = (np.float32(1e-6), np.float32(1.0), np.float32(1e6))
rng = np.random.default_rng(29)
y, x = np.mgrid[0:H, 0:W]
data = np.stack([(280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32) * SCALES[(k + k // 3) % 3]
                 for k in range(14)]).reshape(2, 7, H, W)
opt = ("relative_error_target", 0.004)
THRESHOLD = 285.0


def loop(frames, bins, n_bins, threshold=None, order=None):
    """the reduction of frames [n][rows][cols] (float32), frame after frame"""
    shape = (n_bins,) + frames.shape[1:]
    r = {"sum": np.zeros(shape, np.float64), "sum_sq": np.zeros(shape, np.float64), "min": np.full(shape, np.inf, np.float32),
         "max": np.full(shape, -np.inf, np.float32), "over": np.zeros(shape, np.uint32), "count": np.zeros(n_bins, np.uint64)}
    for f in (range(len(frames)) if order is None else order):
        b = int(bins[f])
        if b < 0:
            continue
        v = frames[f]
        v64 = v.astype(np.float64)
        r["sum"][b] = r["sum"][b] + v64
        r["sum_sq"][b] = r["sum_sq"][b] + v64 * v64
        r["min"][b] = np.minimum(r["min"][b], v) + np.float32(0.0)
        r["max"][b] = np.maximum(r["max"][b], v) + np.float32(0.0)
        if threshold is not None:
            r["over"][b] += v > np.float32(threshold)
        r["count"][b] += 1
    return r


def same(got, want, over):
    for name in ("count", "sum", "sum_sq", "min", "max") + (("over",) if over else ()):
        assert getattr(got, name).tobytes() == want[name].tobytes(), name
    assert over or got.over is None


with h5py.File(os.path.join(out, "r.h5"), "w") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    d = h5_batch.create_dataset(f, "t", data.shape, 20, opt)
    h5_batch.write_frames(d, data, 20, opt, codec=codec)
with h5py.File(os.path.join(out, "r.h5"), "r") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    whole = h5_batch.read_frames(f["t"], codec=codec)
    flat = whole.reshape(-1, H, W)
    # the order of the frames shows in the sums: folded backwards they are other bytes
    assert loop(flat, np.zeros(14, int), 1)["sum"].tobytes() != loop(flat, np.zeros(14, int), 1, order=range(13, -1, -1))["sum"].tobytes()
    got = h5_batch.reduce_frames(f["t"], codec=codec)
    same(got, loop(flat, np.zeros(14, int), 1), False)
    print("OK reduce_frames == the loop over read_frames (one bin, whole frames)")

    bins = np.broadcast_to(np.arange(7) % 3, (2, 7))
    rows, cols = slice(9, 49), slice(50, 80)
    crop = np.ascontiguousarray(whole[..., rows, cols]).reshape(-1, 40, 30)
    want = loop(crop, bins.reshape(-1), 3, THRESHOLD)
    assert want["sum"].tobytes() != loop(crop, bins.reshape(-1), 3, THRESHOLD, order=range(13, -1, -1))["sum"].tobytes()
    assert 0 < want["over"].sum() < 14 * 40 * 30
    h5_batch._SUPER = 1                                              # (four frames a call: the state is carried over four calls)
    got = h5_batch.reduce_frames(f["t"], bins=bins, rows=rows, cols=cols, threshold=THRESHOLD, codec=codec)
    h5_batch._SUPER = 16
    same(got, want, True)
    same(h5_batch.reduce_frames(f["t"], bins=bins, rows=rows, cols=cols, threshold=THRESHOLD, codec=codec), want, True)
    print("OK bins, a window and a threshold: every statistic equals the loop over read_frames()[..., rows, cols]")

    assert got.count.tolist() == [6, 4, 4]
    assert got.mean.dtype == np.float64 and got.mean.tobytes() == (want["sum"] / want["count"].astype(np.float64)[:, None, None]).tobytes()
    m = want["sum"] / want["count"].astype(np.float64)[:, None, None]
    assert got.var.tobytes() == (want["sum_sq"] / want["count"].astype(np.float64)[:, None, None] - m * m).tobytes()
    print("OK mean == sum / count, var == sum_sq / count - mean^2")

    skip = np.array(bins)
    skip[0, 2] = skip[1, 6] = -1
    got = h5_batch.reduce_frames(f["t"], bins=skip, n_bins=4, threshold=THRESHOLD, codec=codec)
    same(got, loop(flat, skip.reshape(-1), 4, THRESHOLD), True)
    assert got.count.tolist() == [5, 4, 3, 0] and np.isnan(got.mean[3]).all() and np.isinf(got.min[3]).all()
    print("OK a -1 bin skips its frame; a bin without frames keeps its initial values")

    for bad in [dict(bins=np.zeros(14, int)), dict(bins=np.full((2, 7), -1)), dict(bins=bins, n_bins=2), dict(bins=bins - 2),
                dict(bins=bins.astype(np.float32)), dict(rows=slice(0, 0))]:
        try:
            h5_batch.reduce_frames(f["t"], codec=codec, **bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad}")
    print("OK bins of another shape, without a frame, beyond n_bins or below -1 are refused")
