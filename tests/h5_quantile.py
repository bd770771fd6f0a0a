"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.quantile_frames against the stated rule -
np.sort over the frames of a bin, the rank rule in float64 - on h5_batch.read_frames.  Prints 'OK' lines;
tests/test_quantile_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ebcc_amd import h5_batch  # noqa: E402

out = sys.argv[1]
H, W = 64, 96
rng = np.random.default_rng(31)
y, x = np.mgrid[0:H, 0:W]
data = np.stack([(280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32)
                 for k in range(24)]).reshape(2, 12, H, W)                     # two "years" of twelve "months"
opt = ("relative_error_target", 0.004)
QS = [0.05, 0.5, 0.95]


def rule(frames, q, method):
    """the quantile of frames [m][rows][cols] (float32) by the stated rule"""
    order = np.sort(frames + np.float32(0), axis=0)
    h = np.float64(q) * np.float64(len(order) - 1)
    fl, ce = int(np.floor(h)), int(np.ceil(h))
    if method != "linear" or fl == ce:
        return order[{"lower": fl, "higher": ce, "nearest": int(np.rint(h)), "linear": fl}[method]]
    lo, hi = order[fl].astype(np.float64), order[ce].astype(np.float64)
    return (lo + (hi - lo) * (h - np.floor(h))).astype(np.float32)


def want(frames, bins, n_bins, method="linear"):
    v = np.full((n_bins, len(QS)) + frames.shape[1:], np.nan, np.float32)
    for b in range(n_bins):
        if (bins == b).any():
            for i, q in enumerate(QS):
                v[b, i] = rule(frames[bins == b], q, method)
    return v


with h5py.File(os.path.join(out, "q.h5"), "w") as f, h5_batch.BatchCodec(H, W, max_frames=5) as codec:
    d = h5_batch.create_dataset(f, "t", data.shape, 20, opt)
    h5_batch.write_frames(d, data, 20, opt, codec=codec)
with h5py.File(os.path.join(out, "q.h5"), "r") as f, h5_batch.BatchCodec(H, W, max_frames=5) as codec:
    whole = h5_batch.read_frames(f["t"], codec=codec)
    flat = whole.reshape(-1, H, W)
    got = h5_batch.quantile_frames(f["t"], QS, codec=codec)
    assert got.values.shape == (1, 3, H, W) and got.count.tolist() == [24]
    assert got.values.tobytes() == want(flat, np.zeros(24, int), 1).tobytes()
    print("OK quantile_frames == the rule on read_frames (one bin, whole frames)")

    season = np.broadcast_to((np.arange(12) % 12) // 3, (2, 12))               # monthly-style bins: four seasons of six frames
    rows, cols = slice(9, 49), slice(50, 80)
    crop = np.ascontiguousarray(whole[..., rows, cols]).reshape(-1, 40, 30)
    for method in ("linear", "nearest"):
        got = h5_batch.quantile_frames(f["t"], QS, bins=season, rows=rows, cols=cols, method=method, codec=codec)
        assert got.count.tolist() == [6, 6, 6, 6]
        assert got.values.tobytes() == want(crop, season.reshape(-1), 4, method).tobytes(), method
    print("OK bins and a window: every quantile equals the rule on read_frames()[..., rows, cols]")

    skip = np.array(season)
    skip[0, 2] = skip[1, 11] = -1
    got = h5_batch.quantile_frames(f["t"], QS, bins=skip, n_bins=5, method="lower", codec=codec)
    assert got.count.tolist() == [5, 6, 6, 5, 0] and np.isnan(got.values[4]).all()
    assert got.values.tobytes() == want(flat, skip.reshape(-1), 5, "lower").tobytes()
    print("OK a -1 bin skips its frame; a bin without frames gives NaN planes")

    for bad in [dict(q=QS, bins=np.zeros(24, int)), dict(q=QS, bins=np.full((2, 12), -1)), dict(q=QS, bins=season, n_bins=2), dict(q=[1.2]),
                dict(q=QS, method="midpoint"), dict(q=QS, rows=slice(0, 0)), dict(q=np.linspace(0.01, 0.99, 17))]:
        try:
            h5_batch.quantile_frames(f["t"], codec=codec, **bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad}")
    print("OK bins of another shape or without a frame, a q outside [0, 1], an unknown method and more than 16 ranks are refused")
