"""CPU tests: the case catalogue of tests/_domains.py against the reference build, and the branches of the two
error-bound searches (src/ebcc_codec.c:545-596 rate search, :730-854 residual / truncation / fallback) it reaches,
read from the oracle's branch trace (orc_last_trace).  The GPU side of the same catalogue is
tests/test_search_branches_gpu.py; the fixture both read is tests/golden/search_branches.json."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import _domains as D
from tests import _lib as L

CASES = D.catalogue()
FIXTURE = json.load(open(os.path.join(L.GOLDEN, "search_branches.json")))["cases"]


def _exit(k, name):
    return lambda t: t["search"][k]["exit"] == name


def _fell_back_for_size(t):
    return t["fallback_smaller"] and not t["fallback_required"]


# Branches the catalogue must reach: name -> predicate on a trace (tests/_lib.py:trace).
BRANCHES = {
    "search0: bisection exit": _exit(0, "bisect"),
    "search0: cr_hi > 1000 exit (no final probe)": _exit(0, "hi_1000"),
    "search0: cr_lo floor": _exit(0, "lo_floor"),
    "search0: could not reach the quantile": lambda t: t["search"][0]["could_not_reach"],
    "search1: bisection exit": _exit(1, "bisect"),
    "search1: cr_hi > 1000 exit (no final probe)": _exit(1, "hi_1000"),
    "search1: cr_lo floor": _exit(1, "lo_floor"),
    "search1: could not reach the quantile": lambda t: t["search"][1]["could_not_reach"],
    "residual: constant field": lambda t: t["residual"] == "const",
    "residual: NONE mode": lambda t: t["residual"] == "mode_none",
    "residual: base meets the bound (skip)": lambda t: t["residual"] == "skip",
    "residual: full SPIHT misses the target (need_pure)": lambda t: t["residual"] == "need_pure",
    "residual: truncation >= 1 step": lambda t: t["residual"] == "trunc" and t["trunc_steps"] >= 1,
    "residual: truncation >= 4 steps": lambda t: t["residual"] == "trunc" and t["trunc_steps"] >= 4,
    "residual layer kept in the stream": lambda t: t["compressed_size"] > 0,
    "fallback: pure base layer because it is smaller": _fell_back_for_size,
    "fallback: pure base layer because it is required": lambda t: t["fallback_required"],
    "mean adjustment applied": lambda t: t["mean_adjusted"],
    "mean adjustment not applied": lambda t: not t["mean_adjusted"],
}

# Branches no input reaches, and why.
UNREACHABLE = {
    "prefix of 1..16 bytes dropped (:811)": (
        lambda t: t["dropped_small"],
        "a kept prefix is a truncation cut or the whole SPIHT stream.  A cut is at least 17 bytes: the loop (:777) needs "
        "trunc_hi - trunc_lo > 32 bits from trunc_lo = 112 (trunc_hi a multiple of 8, so >= 152) and :779 rounds "
        "(152 + 112) / 16 up to 17.  The whole stream codes a residual normalised to [0, 1] (:745) - a 0 and a 1 "
        "somewhere - and is over 100 bytes for the smallest frame the codec takes (32 x 32)."),
}


def _set_quantile(monkeypatch, q):
    monkeypatch.delenv("EBCC_INIT_BASE_ERROR_QUANTILE", raising=False)
    if q is not None:
        monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", q)


def test_trace_layout_matches_the_oracle():
    """tests/_lib.py:OrcTrace mirrors orc_trace_t (oracle/oracle.h) field for field: sizes and offsets as a C compiler
    lays them out on x86-64, read back through a known encode."""
    assert ctypes.sizeof(L.OrcSearchTrace) == 28
    assert [(n, getattr(L.OrcSearchTrace, n).offset) for n, _ in L.OrcSearchTrace._fields_] == [
        ("ran", 0), ("n_halve", 4), ("n_double", 8), ("n_bisect", 12), ("exit", 16), ("could_not_reach", 20), ("result", 24)]
    assert [(n, getattr(L.OrcTrace, n).offset) for n, _ in L.OrcTrace._fields_] == [
        ("n_j2k_encodes", 0), ("n_j2k_decodes", 4), ("n_spiht_decodes", 8), ("final_cr", 12), ("coeffs_size", 16),
        ("compressed_size", 24), ("tail_size", 32), ("search", 40), ("residual", 96), ("trunc_steps", 100),
        ("dropped_small", 104), ("fallback_smaller", 108), ("fallback_required", 112), ("mean_adjusted", 116)]
    assert ctypes.sizeof(L.OrcTrace) == 120
    # a frame whose base layer is exact at every rate: the search doubles past 1000 (30 -> 1920) and stops there
    L.oracle().orc_set_j2k_backend(0)
    x = np.zeros((64, 96), np.float32)
    x[:, 48:] = 1.0
    s = L.orc_encode(x, L.make_config((1, 64, 96), base_cr=30.0, error=0.5))
    t = L.trace()
    assert t["search"][0] == {"ran": 1, "n_halve": 0, "n_double": 6, "n_bisect": 0, "exit": "hi_1000",
                              "could_not_reach": 0, "result": 1920.0}
    assert t["residual"] == "skip" and t["tail_size"] == len(s) - 48 and t["n_j2k_encodes"] >= 7


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_equals_reference_build(case, monkeypatch):
    """Oracle stream == the reference build's stream (live), for every case of the catalogue."""
    if L.reference() is None:
        pytest.skip("reference build (oracle/_ref) not present")
    _set_quantile(monkeypatch, case.quantile)
    L.oracle().orc_set_j2k_backend(0)
    x = case.field()
    cfg = case.config(x)
    got = L.orc_encode(x, cfg)
    assert got == L.ref_encode(x, cfg), (case.name, L.trace())


def _traces():
    return {c.name: FIXTURE[c.name]["trace"] for c in CASES}


def test_catalogue_matches_fixture():
    assert sorted(c.name for c in CASES + [D.overflow_case()]) == sorted(FIXTURE)


def test_catalogue_reaches_every_branch():
    """The union of the traces covers every branch of BRANCHES; a branch no case reaches fails by name (so that an
    edit of the catalogue cannot quietly lose coverage).  The traces are the oracle's (tests/test_oracle_golden.py pins
    them to the fixture)."""
    traces = _traces()
    missing = [b for b, hit in BRANCHES.items() if not any(hit(t) for t in traces.values())]
    assert not missing, f"branches no catalogue case reaches: {missing}"
    for b, (hit, why) in UNREACHABLE.items():
        reached = [n for n, t in traces.items() if hit(t)]
        assert not reached, f"{b!r} is declared unreachable ({why}) but {reached} reach it: move it to BRANCHES"


def test_branch_coverage_uses_the_live_traces(monkeypatch):
    """The fixture's traces are what the oracle reports now (so the coverage above is not a stale record)."""
    L.oracle().orc_set_j2k_backend(0)
    for c in CASES:
        _set_quantile(monkeypatch, c.quantile)
        x = c.field()
        L.orc_encode(x, c.config(x))
        assert L.trace() == FIXTURE[c.name]["trace"], c.name


def feasible(t):
    """The stream this trace describes meets the bound: the base layer alone did (skip), the truncation kept a feasible
    prefix, or the pure base layer was taken from a search that reached quantile 1 (:836)."""
    if t["residual"] in ("const", "mode_none"):
        return t["residual"] == "const"
    if t["fallback_smaller"] or t["fallback_required"]:
        return not t["search"][1]["could_not_reach"]
    return t["residual"] in ("skip", "trunc") and not t["search"][0]["could_not_reach"]


def test_oracle_meets_the_bound_in_float64(monkeypatch):
    """With EBCC_DISABLE_MEAN_ADJUSTMENT=1 (the adjustment, :864-868, can push the max error past the bound - the
    reference does that), every case whose search was feasible decodes within the bound, checked in float64 numpy."""
    monkeypatch.setenv("EBCC_DISABLE_MEAN_ADJUSTMENT", "1")
    L.oracle().orc_set_j2k_backend(0)
    bad = []
    n = 0
    for c in CASES:
        t = FIXTURE[c.name]["trace"]
        if not feasible(t):
            continue
        _set_quantile(monkeypatch, c.quantile)
        x = c.field()
        d = L.orc_decode(L.orc_encode(x, c.config(x))).astype(np.float64)
        e = np.abs(d - x.ravel().astype(np.float64)).max()
        n += 1
        if not e <= c.bound64(x):
            bad.append((c.name, e, c.bound64(x), t))
    assert n >= 40 and not bad, bad


def test_range_overflow_is_refused_by_both():
    """Values at +-3e38: max - min overflows to inf in float32.  The reference scales (x - min) / inf to 0, and inf / inf
    to NaN, then converts to uint16_t (:688) - for NaN an undefined conversion; gcc on x86-64 gives cvttss2si's 0x80000000,
    low half 0, so the image is all 0.  Its decode (s / 65535) * inf + min (:1130) is NaN, so is every residual, and
    spiht_encode stops on assert(dc0 >= 0 && dc0 <= MAXELEM) (spiht_re.c:462): no stream.  Only agreement is pinned -
    the oracle (and the product, tests/test_search_branches_gpu.py) write no stream either."""
    c = D.overflow_case()
    x = c.field()
    with np.errstate(over="ignore"):
        assert np.isfinite(x).all() and np.isinf(np.float32(x.max()) - np.float32(x.min()))
    assert FIXTURE[c.name]["refused"]
    assert L.orc_encode(x, c.config(x)) == b""
    if L.reference() is not None:
        assert D.reference_refuses(c)
