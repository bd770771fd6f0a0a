"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.BatchCodec.series and
h5_batch.series_frames against the numpy restatement of the header's fold (tests/_series.py) on h5_batch.read_frames.  Prints
'OK' lines; tests/test_series_gpu.py drives it."""
import math
import os
import sys

import h5py
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ebcc_amd import h5_batch  # noqa: E402
import _series as S  # noqa: E402

out = sys.argv[1]
H, W = 64, 96
SCALES = (np.float32(1e-6), np.float32(1.0), np.float32(1e6))
rng = np.random.default_rng(31)
y, x = np.mgrid[0:H, 0:W]
data = np.stack([(280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32) * SCALES[(k + k // 3) % 3]
                 for k in range(14)]).reshape(2, 7, H, W)
opt = ("relative_error_target", 0.004)
THRESHOLD = 285.0
REGIONS = [(0, 0, H, W), (9, 50, 40, 30), (H - 1, 0, 1, W), (0, 0, 20, 30), (9, 50, 40, 30)]
w_row = h5_batch.lat_weights(np.linspace(-78.75, 78.75, H))
assert w_row.dtype == np.float64 and w_row.tobytes() == np.cos(np.deg2rad(np.linspace(-78.75, 78.75, H))).tobytes()
w_pix = rng.random((H, W)).astype(np.float32)
w_pix[rng.random((H, W)) < 0.25] = 0.0


def same(got, want, weight):
    for name in S.FIELDS:
        assert getattr(got, name).tobytes() == want[name].tobytes(), name
    assert got.weight.tobytes() == weight.tobytes()


with h5py.File(os.path.join(out, "s.h5"), "w") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    d = h5_batch.create_dataset(f, "t", data.shape, 20, opt)
    h5_batch.write_frames(d, data, 20, opt, codec=codec)
with h5py.File(os.path.join(out, "s.h5"), "r") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    flat = h5_batch.read_frames(f["t"], codec=codec).reshape(-1, H, W)
    # the order of the additions shows in the sums: a plain loop over the pixels gives other bytes
    assert S.region_stats(flat, REGIONS[0], w_row, w_pix)["sum"].tobytes() != S.left_to_right(flat, REGIONS[0], w_row, w_pix).tobytes()

    raw = h5_batch._read_chunks(f["t"], range(14))
    got = codec.series(raw, REGIONS, w_row=w_row, w_pix=w_pix, threshold=THRESHOLD)
    want = S.expected(flat, REGIONS, w_row, w_pix, THRESHOLD)
    weight = S.total_weight(REGIONS, H, W, w_row, w_pix)
    same(got, want, weight)
    assert (got.over[:, 0] > 0).any() and (got.over[:, 0] == 0).any()      # (the frames scaled by 1e-6 stay below the threshold)
    print("OK BatchCodec.series == the fold over read_frames (row and pixel weights, a threshold)")

    h5_batch._SUPER = 1                                              # (four frames a call: four calls, their records concatenated)
    got = h5_batch.series_frames(f["t"], REGIONS, w_row=w_row, w_pix=w_pix, threshold=THRESHOLD, codec=codec)
    h5_batch._SUPER = 16
    same(got, want, weight)
    same(h5_batch.series_frames(f["t"], REGIONS, w_row=w_row, w_pix=w_pix, threshold=THRESHOLD, codec=codec), want, weight)
    print("OK series_frames == BatchCodec.series, whatever the frames a call")

    assert got.mean.dtype == np.float64 and got.mean.tobytes() == (want["sum"] / weight[None, :]).tobytes()
    m = want["sum"] / weight[None, :]
    assert got.var.tobytes() == (want["sum_sq"] / weight[None, :] - m * m).tobytes()
    plain = h5_batch.series_frames(f["t"], REGIONS[:2], codec=codec)
    assert plain.weight.tolist() == [float(H * W), 1200.0] and not plain.over.any()
    same(plain, S.expected(flat, REGIONS[:2]), np.array([H * W, 1200.0]))
    rows_only = h5_batch.series_frames(f["t"], REGIONS[:2], w_row=w_row, codec=codec)
    assert rows_only.weight[0] == math.fsum(np.repeat(w_row, W).tolist())
    print("OK weight is the order-free total, mean == sum / weight, var == sum_sq / weight - mean^2")

    pick = [13, 0, 5, 5, 2]
    got = h5_batch.series_frames(f["t"], REGIONS, frames=pick, w_row=w_row, codec=codec)
    same(got, S.expected(flat[pick], REGIONS, w_row), S.total_weight(REGIONS, H, W, w_row))
    for bad in [dict(regions=[(0, 0, H + 1, W)]), dict(regions=[]), dict(regions=[(0, 0, 0, 4)]), dict(regions=REGIONS, frames=[14]),
                dict(regions=REGIONS, frames=[]), dict(regions=REGIONS, w_row=-w_row), dict(regions=REGIONS, w_row=w_row[:-1]),
                dict(regions=REGIONS, w_pix=w_pix[:, :-1])]:
        try:
            h5_batch.series_frames(f["t"], codec=codec, **bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad}")
    nan = w_pix.copy()
    nan[3, 3] = np.nan
    try:
        h5_batch.series_frames(f["t"], REGIONS, w_pix=nan, codec=codec)
        raise AssertionError("accepted a NaN weight")
    except RuntimeError as e:
        assert "d_w_pix" in str(e)
    print("OK frames in any order; regions, frames and weights the engine refuses are refused")
