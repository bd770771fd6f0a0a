"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.write_variables - several datasets with
their own filter parameters coded in one device call - against h5_batch.write_frames dataset by dataset.  Prints 'OK' lines;
tests/test_group_encode_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ebcc_amd import h5_batch  # noqa: E402

out = sys.argv[1]
H, W = 70, 100
rng = np.random.default_rng(9)
y, x = np.mgrid[0:H, 0:W]
t = np.stack([(280 + 10 * np.sin(x / (9.0 + k)) * np.cos(y / (7.0 + k)) + rng.normal(0, 0.4, (H, W))).astype(np.float32) for k in range(5)])
q = np.stack([(0.01 + 0.004 * np.cos(x / (6.0 + k)) + rng.normal(0, 2e-4, (H, W))).astype(np.float32) for k in range(6)]).reshape(2, 3, H, W)
t[2] = 1.5                                                       # constant field
VARS = {"t": (t, 20, ("max_error_target", 0.1)), "q": (q, 8, ("relative_error_target", 0.01)), "mask": (t[:2] > 280, 15, ("none", None))}


def chunks(d):
    lead = d.shape[:-2]
    return [d.id.read_direct_chunk(tuple(int(v) for v in np.unravel_index(k, lead)) + (0, 0))[1] for k in range(int(np.prod(lead)))]


# dataset by dataset
with h5py.File(os.path.join(out, "one.h5"), "w") as f:
    for name, (data, cr, opt) in VARS.items():
        h5_batch.write_frames(h5_batch.create_dataset(f, name, data.shape, cr, opt), data.astype(np.float32), cr, opt)
with h5py.File(os.path.join(out, "one.h5"), "r") as f:
    want = {name: chunks(f[name]) for name in VARS}
    back = {name: f[name][...] for name in VARS}

# all of them in one device call; `t` in two items, the second beginning at frame 3
with h5py.File(os.path.join(out, "all.h5"), "w") as f:
    d = {name: h5_batch.create_dataset(f, name, data.shape, cr, opt) for name, (data, cr, opt) in VARS.items()}
    assert h5_batch.filter_options(d["q"]) == (8.0, ("relative_error_target", float(np.float32(0.01))))
    assert h5_batch.filter_options(d["mask"]) == (15.0, ("none", None))
    h5_batch.write_variables([(d["t"], 0, t[:3]), (d["q"], 0, q.reshape(-1, H, W)), (d["mask"], 0, VARS["mask"][0].astype(np.float32)),
                              (d["t"], 3, t[3:])])
    try:
        h5_batch.write_variables([(d["t"], 4, t[:3])])
        raise SystemExit("frames past the end of the dataset were accepted")
    except ValueError:
        pass
print("OK write_variables")
with h5py.File(os.path.join(out, "all.h5"), "r") as f:
    got = {name: chunks(f[name]) for name in VARS}
    assert got == want, {name: [len(a) - len(b) for a, b in zip(got[name], want[name])] for name in VARS}
    print("OK chunk bytes == write_frames per dataset", sum(len(c) for v in got.values() for c in v))
    for name in VARS:
        assert np.array_equal(h5_batch.read_frames(f[name]), back[name]), name
    assert np.abs(back["t"] - t).max() <= 0.1 * 1.01 + 1e-4
print("OK read_frames of every variable")
