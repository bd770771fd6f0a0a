"""The hard-bound direct-chunk write and the audit of a dataset (ebcc_amd/h5_batch.py: write_frames(hard=True), audit_dataset)
through h5py from the image's conda, driven as tests/test_hdf5_gpu.py drives h5_roundtrip.py: tests/h5_hard_write.py writes the
64 x 96 MAX_ERROR 0.02 set (tests/_hard_bound.py) softly and hard, audits both files and reads the hard one through the plain
filter callback; the reports it leaves are then held against the rule restated on the oracle."""
import os
import subprocess

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L

CONDA_PY = "/opt/conda/bin/python3.9"


@pytest.mark.gpu
def test_hard_write_and_audit_dataset(tmp_path, monkeypatch):
    from ebcc_amd import h5_batch
    assert callable(h5_batch.audit_dataset) and callable(h5_batch.BatchCodec.audit)      # (missing: a failure, not a skip)
    if not os.path.exists(CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    HB.use_env(monkeypatch, {})
    x = HB.set_inputs("max_64x96")
    np.save(tmp_path / "data.npy", x)
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([CONDA_PY, os.path.join(L.ROOT, "tests", "h5_hard_write.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 4, r.stdout
    loop = HB.set_loop("max_64x96")
    report = np.load(tmp_path / "report.npy")
    for f, (_s, rep, _h) in enumerate(loop):
        assert tuple(report[f]) == tuple(rep), (f, report[f], rep)
    soft = np.load(tmp_path / "soft_audit.npy")
    assert np.flatnonzero(soft["n_over"]).tolist() == [1, 3]
    hard = np.load(tmp_path / "hard_audit.npy")
    assert (hard["n_over"] == 0).all() and hard["max_abs"].tobytes() == report["achieved"].tobytes()
