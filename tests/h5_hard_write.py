"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: a hard-bound direct-chunk write
(h5_batch.write_frames(hard=True)), the audit of the file against the data (h5_batch.audit_dataset), and the same chunks read
through the plain HDF5 filter callback.  argv[1]: a directory holding data.npy, (n, H, W) float32, written to as well.  Prints
'OK' lines; tests/test_hard_write_hdf5_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ebcc_amd import h5_batch  # noqa: E402

out = sys.argv[1]
data = np.load(os.path.join(out, "data.npy"))
cr, err = 20, 0.02
opt = ("max_error_target", err)

# (1) the soft write: the audit finds the frames a reader gets outside the bound
with h5py.File(os.path.join(out, "soft.h5"), "w") as f:
    d = h5_batch.create_dataset(f, "t", data.shape, cr, opt)
    assert h5_batch.write_frames(d, data, cr, opt) is None
with h5py.File(os.path.join(out, "soft.h5"), "r") as f:
    soft = h5_batch.audit_dataset(f["t"], data)
    soft_raw = [f["t"].id.read_direct_chunk((k, 0, 0))[1] for k in range(len(data))]
np.save(os.path.join(out, "soft_audit.npy"), soft)
print("OK soft write audited, frames over the bound:", np.flatnonzero(soft["n_over"]).tolist())

# (2) the hard write: every frame inside its bound, for the audit and for the plain filter callback
with h5py.File(os.path.join(out, "hard.h5"), "w") as f:
    d = h5_batch.create_dataset(f, "t", data.shape, cr, opt)
    report = h5_batch.write_frames(d, data, cr, opt, hard=True)
with h5py.File(os.path.join(out, "hard.h5"), "r") as f:
    audit = h5_batch.audit_dataset(f["t"], data)
    back = f["t"][...]                                           # (the filter callback, one chunk per call)
    hard_raw = [f["t"].id.read_direct_chunk((k, 0, 0))[1] for k in range(len(data))]
np.save(os.path.join(out, "report.npy"), report)
np.save(os.path.join(out, "hard_audit.npy"), audit)
assert report.shape == (len(data),) and (report["met"] == 1).all()
assert (audit["n_over"] == 0).all() and (audit["max_abs"] <= np.float32(err)).all(), audit["max_abs"]
print("OK hard write: every frame inside its bound, worst", float(audit["max_abs"].max()), "rounds", report["rounds"].tolist())
seen = np.abs(back - data).reshape(len(data), -1).max(axis=1)
assert seen.dtype == np.float32 and seen.tobytes() == audit["max_abs"].tobytes() and report["achieved"].tobytes() == seen.tobytes(), (seen, audit["max_abs"])
assert (seen <= np.float32(err)).all()
print("OK the chunks decode through the filter callback to what the audit measured")
assert all((hard_raw[k] == soft_raw[k]) == (report["rounds"][k] == 0) for k in range(len(data)))
print("OK frames that met the bound at once keep the plain write's chunk bytes")
