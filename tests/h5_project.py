"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.project_frames against the same map -
a loop over every output's terms in increasing frame, acc = acc + weight * float64(x) - of h5_batch.read_frames.  Prints 'OK'
lines; tests/test_time_map_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ebcc_amd import h5_batch  # noqa: E402

out = sys.argv[1]
H, W = 64, 96
SCALES = (np.float32(1e-6), np.float32(1.0), np.float32(1e6))
rng = np.random.default_rng(31)
y, x = np.mgrid[0:H, 0:W]
data = np.stack([(280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32) * SCALES[(k + k // 3) % 3]
                 for k in range(14)]).reshape(2, 7, H, W)
opt = ("relative_error_target", 0.004)


def loop(frames, terms, order=1):
    """the map of frames [n][rows][cols] (float32), term after term; order -1: every output's terms backwards"""
    start, frame, weight = terms
    acc = np.zeros((len(start) - 1,) + frames.shape[1:], np.float64)
    for o in range(len(start) - 1):
        for t in range(int(start[o]), int(start[o + 1]))[::order]:
            acc[o] = acc[o] + weight[t] * frames[frame[t]].astype(np.float64)
    return acc


with h5py.File(os.path.join(out, "p.h5"), "w") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    d = h5_batch.create_dataset(f, "t", data.shape, 20, opt)
    h5_batch.write_frames(d, data, 20, opt, codec=codec)
with h5py.File(os.path.join(out, "p.h5"), "r") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    whole = h5_batch.read_frames(f["t"], codec=codec)
    flat = whole.reshape(-1, H, W)
    trend = h5_batch.trend_weights(np.arange(14.0) * 0.25 + 1979.0)
    terms = h5_batch.time_map_terms(trend)
    want = loop(flat, terms)
    assert want.tobytes() != loop(flat, terms, -1).tobytes()         # the order of the frames shows in the sums
    got = h5_batch.project_frames(f["t"], trend, codec=codec)
    assert got.values.dtype == np.float64 and got.values.tobytes() == want.tobytes() and got.count.tolist() == [14, 14]
    print("OK project_frames == the loop over read_frames (the trend map, whole frames)")

    rows, cols = slice(9, 49), slice(50, 80)
    crop = np.ascontiguousarray(whole[..., rows, cols]).reshape(-1, 40, 30)
    band = h5_batch.running_mean_weights(14, 5) * np.array([1.0, -2.0 / 7.0, 0.3])[np.arange(10) % 3][:, None]
    want = loop(crop, h5_batch.time_map_terms(band))
    h5_batch._SUPER = 1                                              # (four frames a call: the state is carried over four calls)
    got = h5_batch.project_frames(f["t"], band, rows=rows, cols=cols, codec=codec)
    h5_batch._SUPER = 16
    assert got.values.tobytes() == want.tobytes() and got.count.tolist() == [5] * 10
    assert h5_batch.project_frames(f["t"], band, rows=rows, cols=cols, codec=codec).values.tobytes() == want.tobytes()
    print("OK a banded map and a window, walked in four calls and in one")

    sparse = (np.array([0, 3, 3, 5]), np.array([1, 6, 12, 6, 13]), np.array([1.0 / 3.0, -2.0 / 7.0, 0.1, 1e3, -1e-3]))
    reads = []
    real = h5_batch._read_chunks
    h5_batch._read_chunks = lambda dset, frames: reads.extend(int(v) for v in frames) or real(dset, frames)
    h5_batch._SUPER = 1
    got = h5_batch.project_frames(f["t"], sparse, codec=codec)
    h5_batch._SUPER, h5_batch._read_chunks = 16, real
    assert got.values.tobytes() == loop(flat, sparse).tobytes() and got.count.tolist() == [3, 0, 2]
    assert reads == [1, 6, 12, 13] and not got.values[1].any()
    print("OK a sparse triple: only the named frames' chunks are fetched, an output without terms stays 0")

    for bad in [np.zeros((2, 14)), np.ones((2, 13)), (np.array([0, 1]), np.array([14]), np.array([1.0])),
                (np.array([0, 2]), np.array([3, 3]), np.array([1.0, 1.0])), np.full((1, 14), np.nan)]:
        try:
            h5_batch.project_frames(f["t"], bad, codec=codec)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad}")
    try:
        h5_batch.project_frames(f["t"], trend, rows=slice(0, 0), codec=codec)
        raise AssertionError("accepted an empty window")
    except ValueError:
        pass
    print("OK a map without terms, of another length, beyond the frames, out of order or not finite is refused")
