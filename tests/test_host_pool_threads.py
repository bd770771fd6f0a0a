"""CPU test of product code: the process-wide worker pool (HostPool, ebcc_amd/csrc/host.hpp - the class the library's entropy
stage runs on) fed by four caller threads at once, in a stand-alone host program with its own main
(tests/host_pool_threads.cpp; the host half of a HIP compile, no device call).  Once plain: every job of every batch runs
exactly once, a throwing job fails its own batch alone.  Once under the thread sanitizer, linked into that program itself:
no data race is reported."""
import os
import subprocess

import pytest

from tests import _lib as L

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("sanitizer", [None, "thread"])
def test_host_pool_under_four_callers(tmp_path, sanitizer):
    exe = str(tmp_path / "host_pool_threads")
    flags = ["-O1", "-g", "-fsanitize=" + sanitizer] if sanitizer else ["-O2"]
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-Wno-option-ignored", *flags,
                           "-I" + os.path.join(L.ROOT, "include"), "-o", exe, os.path.join(L.ROOT, "tests", "host_pool_threads.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    if sanitizer and "FATAL: ThreadSanitizer" in out:
        pytest.skip("the sanitizer's runtime cannot start in this environment: " + out.strip().splitlines()[0])
    assert "ThreadSanitizer" not in out, out[-3000:]
    assert r.returncode == 0 and "0 failures" in out, out[-3000:]
