"""CPU test: the reference of the probe tests (tests/_probes.py) against the oracle's whole encode.

For the catalogue cases whose encode runs the truncation bisection (src/ebcc_codec.c:765-796), with the pure base-layer
fallback off so that the residual layer stays in the stream: the base layer rebuilt at the rate the oracle's search ended on,
the residual layer rebuilt from it, and the restated bisection over the restated per-cut maxima must visit as many cuts as
the oracle did and end on its prefix - whose bytes, with the residual range, are then read back out of the oracle's stream.
tests/test_probe_residual_gpu.py and tests/test_probe_j2k_gpu.py compare the product's probes with this reference."""
import json
import os

import numpy as np
import pytest

from tests import _domains as D
from tests import _lib as L
from tests import _probes as P

FIXTURE = json.load(open(os.path.join(L.GOLDEN, "search_branches.json")))["cases"]
TRUNC = [c for c in D.catalogue() if FIXTURE[c.name]["trace"]["residual"] == "trunc"]
# a spread over the domains and the three shapes, the longest bisections first
CASES = sorted(TRUNC, key=lambda c: -FIXTURE[c.name]["trace"]["trunc_steps"])[:10]


def test_enough_cases():
    assert len(CASES) >= 6
    assert len({c.shape for c in CASES}) >= 2 and max(FIXTURE[c.name]["trace"]["trunc_steps"] for c in CASES) >= 4


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_restates_the_oracle(case, monkeypatch):
    monkeypatch.setenv("EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "1")
    monkeypatch.delenv("EBCC_INIT_BASE_ERROR_QUANTILE", raising=False)
    if case.quantile is not None:
        monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", case.quantile)
    L.oracle().orc_set_j2k_backend(0)
    x = case.field()
    stream = L.orc_encode(x, case.config(x))
    t = L.trace()
    assert t["residual"] == "trunc" and t["trunc_steps"] >= 1 and t["coeffs_size"] > 16, t
    # the base layer the residual was taken against (:728) and the budget it sets (:747)
    d, base_bytes = P.base_layer(x, t["final_cr"])
    assert base_bytes == t["tail_size"]
    res = P.Residual(x, d, 8 * base_bytes)
    target = case.target(x)
    assert res.maxerr(len(res.stream)) <= target                              # :755: the whole stream is feasible
    visited, coeffs_size = P.bisection(res.maxerr, len(res.stream), target)
    assert len(visited) == t["trunc_steps"], (visited, t)
    assert coeffs_size == t["coeffs_size"], (coeffs_size, t)
    rmin, rmax, prefix = P.frame_stream_parts(stream)
    assert P.f32_bits(rmin) == P.f32_bits(res.rmin) and P.f32_bits(rmax) == P.f32_bits(res.rmax)
    assert prefix == res.stream[:coeffs_size]
    assert res.maxerr(coeffs_size) <= target                                  # the kept cut is within the target


def test_bisection_ladder_and_bounds():
    """the helpers the GPU tests lean on"""
    cuts = P.ladder(1600)
    assert cuts[0] == 17 and cuts[-1] == 1600 and set(range(17, 273)) <= set(cuts) and set(range(1537, 1601)) <= set(cuts)
    assert 330 < len(cuts) < 420 and cuts == sorted(set(cuts))
    assert P.ladder(100) == list(range(17, 101))
    e = np.array([1.0, -1.0, 2.0 ** -30], np.float32)
    assert P.error_sum(e) == 2.0 ** -30 and P.sum_bound(e) == 3 * 2.0 ** -52 * (2 + 2.0 ** -30)
    # a maximum equal to the target is feasible (:784 is a strict comparison), and the loop ends at once on it (:777)
    visited, size = P.bisection(lambda c: np.float32(0.5), 400, 0.5)
    assert visited == [] and size == 400
    # a non-monotone profile: feasible at the end, infeasible in the middle, feasible again early - the bisection goes by what
    # it sees (first cut (3200 + 112) / 2 -> 207 bytes)
    prof = lambda c: np.float32(0.1 if c >= 300 or c < 120 else 0.9)
    visited, size = P.bisection(prof, 400, 0.5)
    assert visited[0] == 207 and prof(size) <= 0.5 and size >= 300
