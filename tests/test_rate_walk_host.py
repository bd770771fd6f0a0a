"""CPU test of product code: the pass walk of the rate allocation and its per-code-block walk tables
(ebcc_amd/csrc/rate_walk.hpp, the very source the gfx950 kernels compile) built for the host.  The table's answer must
equal the greedy walk at every limit, next to it and at random thresholds; see tests/rate_walk_host_check.cpp.  Run once
as a plain build and once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is
preloaded)."""
import os
import subprocess

import pytest

from tests import _lib as L

SRC = os.path.join(L.ROOT, "tests", "rate_walk_host_check.cpp")


@pytest.mark.parametrize("flags,n", [((), "3000"), (("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"), "600")],
                         ids=["plain", "sanitized"])
def test_walk_tables_match_the_walk(tmp_path, flags, n):
    exe = str(tmp_path / "rate_walk_host_check")
    # -ffp-contract=off: the arithmetic of the device build (ebcc_amd/csrc/Makefile)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, SRC])
    res = subprocess.run([exe, n], capture_output=True, text=True)
    assert res.returncode == 0 and " 0 failures" in res.stdout, res.stdout + res.stderr
