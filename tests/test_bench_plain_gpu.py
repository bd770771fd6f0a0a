"""bench.py without --full: the headline line alone, --steps timed steps, and --dump-outputs writing the last timed step's
results as float arrays that are the same from run to run (seeded inputs, a deterministic codec)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _lib as L

pytestmark = pytest.mark.gpu

FULL_ONLY = ("max_abs_error", "kernels", "roofline", "roofline_decode", "host", "cpu_baseline", "config3", "shard4096")


def run_plain(tmp_path, tag):
    d = tmp_path / tag
    cmd = [sys.executable, os.path.join(L.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "12",
           "--dump-outputs", str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-600:], r.stderr[-1200:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), d


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    line, d = run_plain(tmp_path, "a")
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 2 and line["config"]["frames_per_gpu"] == 12
    assert abs(line["value"] - 12 * 721 * 1440 * 4 / (line["ms_per_step"] * 1e-3) / 1e9) < 1e-3 * line["value"] + 1e-4
    assert not [k for k in FULL_ONLY if k in line]
    files = sorted(os.listdir(d))
    assert files == ["decoded_frame_index.npy", "decoded_frames.npy", "decoded_sample.npy", "stream_bytes.npy", "stream_sha256.npy"]
    arrays = {f[:-4]: np.load(d / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    assert arrays["decoded_frames"].shape == (8, 721, 1440) and arrays["stream_sha256"].shape == (12, 32)
    assert int(arrays["stream_bytes"].sum()) // 12 == line["compressed_bytes_per_frame"]
    assert np.isfinite(arrays["decoded_frames"]).all() and 150 < float(arrays["decoded_sample"].mean()) < 350

    _, d2 = run_plain(tmp_path, "b")                            # same arguments: same inputs, same outputs
    for name, a in arrays.items():
        assert np.array_equal(a, np.load(d2 / (name + ".npy"))), name
