"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.pair_frames on two datasets against
the same loop - step after step in order, in float64 / float32 as include/ebcc_hip.h states it - over h5_batch.read_frames of
both.  Prints 'OK' lines; tests/test_pair_gpu.py drives it."""
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


def field(k, s):
    return (280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32) * SCALES[s % 3]


# (steps 2, 5, 8, .. pair fields of equal scale, the others differ by 1e6)
u = np.stack([field(k, k + k // 3) for k in range(10)]).reshape(2, 5, H, W)
v = np.stack([field(k + 20, k + k // 3 + (k % 3 != 2)) for k in range(10)]).reshape(2, 5, H, W)
opt = ("relative_error_target", 0.004)
THRESHOLD = 300.0
NAMES = ("sum_x", "sum_y", "sum_xx", "sum_yy", "sum_xy", "sum_mag")


def loop(fx, fy, bins, n_bins, threshold=None, order=None):
    """the pair statistics of fx, fy [n][rows][cols] (float32), step after step"""
    shape = (n_bins,) + fx.shape[1:]
    r = {name: np.zeros(shape, np.float64) for name in NAMES}
    r.update({"max_mag": np.full(shape, -np.inf, np.float32), "over_mag": np.zeros(shape, np.uint32), "count": np.zeros(n_bins, np.uint64)})
    for t in (range(len(fx)) if order is None else order):
        k = int(bins[t])
        if k < 0:
            continue
        a, b = fx[t].astype(np.float64), fy[t].astype(np.float64)
        m = np.sqrt((a * a + b * b).astype(np.float32))
        for name, term in zip(NAMES, (a, b, a * a, b * b, a * b, m.astype(np.float64))):
            r[name][k] = r[name][k] + term
        r["max_mag"][k] = np.maximum(r["max_mag"][k], m)
        if threshold is not None:
            r["over_mag"][k] += m > np.float32(threshold)
        r["count"][k] += 1
    return r


def same(got, want, over, magnitude=True):
    for name in ("count",) + NAMES[:5] + (("sum_mag", "max_mag") if magnitude else ()) + (("over_mag",) if over else ()):
        assert getattr(got, name).tobytes() == want[name].tobytes(), name
    assert over or got.over_mag is None
    assert magnitude or (got.sum_mag is None and got.max_mag is None)


with h5py.File(os.path.join(out, "p.h5"), "w") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    for name, data in (("u", u), ("v", v)):
        d = h5_batch.create_dataset(f, name, data.shape, 20, opt)
        h5_batch.write_frames(d, data, 20, opt, codec=codec)
    h5_batch.create_dataset(f, "short", (2, 4, H, W), 20, opt)
with h5py.File(os.path.join(out, "p.h5"), "r") as f, h5_batch.BatchCodec(H, W, max_frames=3) as codec:
    fu, fv = h5_batch.read_frames(f["u"], codec=codec), h5_batch.read_frames(f["v"], codec=codec)
    flat_u, flat_v = fu.reshape(-1, H, W), fv.reshape(-1, H, W)
    zeros = np.zeros(10, int)
    want = loop(flat_u, flat_v, zeros, 1)
    # the order of the steps shows in the sums: folded backwards they are other bytes
    assert want["sum_xy"].tobytes() != loop(flat_u, flat_v, zeros, 1, order=range(9, -1, -1))["sum_xy"].tobytes()
    got = h5_batch.pair_frames(f["u"], f["v"], codec=codec)         # (capacity 3: one step a batch)
    same(got, want, False)
    print("OK pair_frames == the loop over read_frames of both datasets (one bin, whole frames)")

    bins = np.broadcast_to(np.arange(5) % 3, (2, 5)).copy()
    bins[1, 3] = -1
    rows, cols = slice(9, 49), slice(50, 80)
    cu, cv = (np.ascontiguousarray(a[..., rows, cols]).reshape(-1, 40, 30) for a in (fu, fv))
    want = loop(cu, cv, bins.reshape(-1), 4, THRESHOLD)
    assert 0 < want["over_mag"].sum() < 9 * 40 * 30
    h5_batch._SUPER = 1                                              # (one step a call: the state is carried over nine calls)
    got = h5_batch.pair_frames(f["u"], f["v"], bins=bins, n_bins=4, rows=rows, cols=cols, threshold=THRESHOLD, codec=codec)
    h5_batch._SUPER = 16
    same(got, want, True)
    same(h5_batch.pair_frames(f["u"], f["v"], bins=bins, n_bins=4, rows=rows, cols=cols, threshold=THRESHOLD), want, True)    # (the cached codec)
    assert got.count.tolist() == [3, 4, 2, 0]
    print("OK bins with a skipped step, a window and a threshold: every array equals the loop over read_frames()[..., rows, cols]")

    n = want["count"].astype(np.float64)[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_u, mean_v = want["sum_x"] / n, want["sum_y"] / n
        assert got.mean_x[:3].tobytes() == mean_u[:3].tobytes() and got.mean_y[:3].tobytes() == mean_v[:3].tobytes()
        assert got.cov[:3].tobytes() == (want["sum_xy"] / n - mean_u * mean_v)[:3].tobytes()
        assert got.mean_mag[:3].tobytes() == (want["sum_mag"] / n)[:3].tobytes()
    r = got.corr
    assert r.dtype == np.float64 and np.isfinite(r[:3]).any() and (np.abs(r[np.isfinite(r)]) <= 1 + 1e-9).all()
    assert all(np.isnan(a[3]).all() for a in (got.mean_x, got.mean_y, got.cov, r, got.mean_mag))
    bare = h5_batch.pair_frames(f["u"], f["u"], magnitude=False, codec=codec)
    same(bare, loop(flat_u, flat_u, zeros, 1), False, magnitude=False)
    assert bare.sum_xy.tobytes() == bare.sum_xx.tobytes() and bare.mean_mag is None
    print("OK means, cov and corr; corr lies in [-1, 1]; a bin without steps gives NaN; a dataset with itself, co-moments only")

    for bad in [dict(bins=np.zeros(10, int)), dict(bins=np.full((2, 5), -1)), dict(bins=bins, n_bins=2), dict(bins=bins - 2),
                dict(bins=bins.astype(np.float32)), dict(rows=slice(0, 0)), dict(threshold=1.0, magnitude=False)]:
        try:
            h5_batch.pair_frames(f["u"], f["v"], codec=codec, **bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad}")
    try:
        h5_batch.pair_frames(f["u"], f["short"], codec=codec)
    except ValueError:
        pass
    else:
        raise AssertionError("accepted datasets of different shape")
    print("OK datasets of different shape and bad bins are refused")
