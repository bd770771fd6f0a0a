"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.read_regridded and
h5_batch.BatchCodec.regrid against the numpy restatement of the header's rule (tests/_regrid.py) on h5_batch.read_frames.
Prints 'OK' lines; tests/test_regrid_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ebcc_amd import h5_batch  # noqa: E402
from ebcc_amd import regrid as M  # noqa: E402
import _regrid as R  # noqa: E402

out = sys.argv[1]
H, W = 64, 96
SCALES = (np.float32(1e-6), np.float32(1.0), np.float32(1e6))
rng = np.random.default_rng(37)
y, x = np.mgrid[0:H, 0:W]
data = np.stack([(280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32) * SCALES[(k + k // 3) % 3]
                 for k in range(12)]).reshape(2, 6, H, W)
opt = ("relative_error_target", 0.004)
lat, lon = np.linspace(78.75, -78.75, H), np.arange(W) * 3.75
MAPS = {"1 : 4 conservative, periodic columns": (M.conservative_map(M.cell_edges(lat), M.cell_edges(lat[::4] - 3.75), measure=lambda e: np.sin(np.deg2rad(e))),
                                                 M.conservative_map(M.cell_edges(lon), M.cell_edges(lon[::4]), period=360.0)),
        "a window": (M.conservative_map(np.arange(H + 1.0), np.linspace(10.0, 50.0, 8)), M.block_mean_map(W, 4, weights=np.arange(1.0, W + 1))),
        "flip and interpolate": (M.flip_map(H), M.linear_map(lon, np.linspace(0.0, 359.0, 50), period=360.0))}
assert MAPS["1 : 4 conservative, periodic columns"][1].wrap and MAPS["flip and interpolate"][1].wrap

with h5py.File(os.path.join(out, "g.h5"), "w") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    d = h5_batch.create_dataset(f, "t", data.shape, 20, opt)
    h5_batch.write_frames(d, data, 20, opt, codec=codec)
with h5py.File(os.path.join(out, "g.h5"), "r") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    flat = h5_batch.read_frames(f["t"], codec=codec).reshape(-1, H, W)
    raw = h5_batch._read_chunks(f["t"], range(12))
    for name, (rows, cols) in MAPS.items():
        want = R.apply(flat, rows, cols)
        got = codec.regrid(raw, rows, cols)
        assert got.dtype == np.float32 and got.shape == (12, rows.n_out, cols.n_out) and got.tobytes() == want.tobytes(), name
    print("OK BatchCodec.regrid == the rule over read_frames (three batches on two engine sets)")

    for name, (rows, cols) in MAPS.items():
        want = R.apply(flat, rows, cols)
        h5_batch._SUPER = 1                                          # (four frames a call: three calls)
        got = h5_batch.read_regridded(f["t"], rows, cols, codec=codec)
        h5_batch._SUPER = 16
        assert got.tobytes() == want.tobytes(), name
        assert h5_batch.read_regridded(f["t"], rows, cols, codec=codec).tobytes() == want.tobytes(), name
        assert h5_batch.read_regridded(f["t"], rows, cols).tobytes() == want.tobytes(), name       # (a codec of its own)
    print("OK read_regridded == BatchCodec.regrid, whatever the frames a call")

    rows, cols = MAPS["a window"]
    pick = [11, 0, 5, 5, 2]
    assert h5_batch.read_regridded(f["t"], rows, cols, frames=pick, codec=codec).tobytes() == R.apply(flat[pick], rows, cols).tobytes()
    for bad in [dict(row_map=M.identity_map(H + 1), col_map=cols), dict(row_map=rows, col_map=cols, frames=[12]), dict(row_map=rows, col_map=cols, frames=[]),
                dict(row_map=M.AxisMap([0], [1], [1.0], wrap=True), col_map=cols)]:
        try:
            h5_batch.read_regridded(f["t"], codec=codec, **bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad}")
    print("OK frames in any order; maps and frames the engine refuses are refused")
