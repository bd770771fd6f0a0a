"""GPU: two quantile calls at once on one context get the bytes a serial caller gets.

The select keeps its counters, prefixes and remaining ranks in the context from its first pass to its last, so
ebcc_hip_quantile_shard and ebcc_hip_rank_items hold the device's lock over all eight passes (thread safety).
One fresh child process - `python -m tests._quantile_threads`, see that module - runs the scenario, as tests/test_threads_gpu.py
runs its own."""
import os
import subprocess
import sys

import pytest

from tests import _hard_bound as HB
from tests import _lib as L

pytestmark = pytest.mark.gpu

LIMIT = 600                                           # seconds: what the suite's other child processes get


def test_two_quantile_calls_of_different_sizes_on_one_context():
    """One thread selects three bins of whole frames, the other one bin of a window and then the kernels alone on four bins, three
    rounds each, on the ONE ctx.  Were the lock given up between passes, one call's start values would wipe the other's
    counters and prefixes in mid-select: wrong planes."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("EBCC_HIP_") and k not in HB.ENV_NAMES}
    try:
        r = subprocess.run([sys.executable, "-m", "tests._quantile_threads"], capture_output=True, text=True, env=env, cwd=L.ROOT, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"no end within {LIMIT} s - a deadlock?  The child's trail:\n{out}")
    lines = r.stdout.strip().splitlines()
    print("\n".join(lines))
    assert r.returncode == 0 and lines and lines[-1] == "compared", (r.returncode, lines, r.stderr[-2000:])
