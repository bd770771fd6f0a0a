"""GPU: the case catalogue of tests/_domains.py (value domains x error targets x start rates x quantiles, chosen to take
every branch of the two error-bound searches - tests/test_search_branches.py) through the MI355X codec: one frame at a
time, in batches whose frames finish their searches in different rounds, and under the search's build-time-free
variants.  Streams against the reference build's (tests/golden/search_branches.json), decoded fields against the
oracle's decode of the same stream, and the bound itself checked in float64."""
import ctypes
import hashlib
import json
import os
from collections import defaultdict

import numpy as np
import pytest

from tests import _domains as D
from tests import _lib as L
from tests.test_search_branches import feasible

pytestmark = pytest.mark.gpu

CASES = D.catalogue()
FIXTURE = json.load(open(os.path.join(L.GOLDEN, "search_branches.json")))["cases"]
VARIANTS = [{"EBCC_HIP_SEARCH_ROUNDS": "2"}, {"EBCC_HIP_TRUNC_LEVELS": "1"}, {"EBCC_HIP_TRUNC_LEVELS": "3"},
            {"EBCC_HIP_SPECULATION": "0"}]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def encode(x, cfg):
    """ebcc_encode of the product (b"" when it writes no stream)"""
    lib = L.product()
    x = np.ascontiguousarray(x, np.float32)
    out = ctypes.c_void_p()
    n = lib.ebcc_encode(x.ctypes.data, ctypes.byref(cfg), ctypes.byref(out))
    if n == 0:
        return b""
    s = ctypes.string_at(out.value, n)
    lib.free_buffer(out)
    return s


def decode(s):
    lib = L.product()
    b = ctypes.create_string_buffer(bytes(s), len(s))
    out = ctypes.c_void_p()
    n = lib.ebcc_decode(b, len(s), ctypes.byref(out))
    assert n > 0
    a = np.frombuffer(ctypes.string_at(out.value, 4 * n), np.float32).copy()
    lib.free_buffer(out)
    return a


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _env(monkeypatch, quantile, extra=()):
    for k in ["EBCC_INIT_BASE_ERROR_QUANTILE", "EBCC_DISABLE_MEAN_ADJUSTMENT"] + [k for v in VARIANTS for k in v]:
        monkeypatch.delenv(k, raising=False)
    if quantile is not None:
        monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", quantile)
    for k, v in dict(extra).items():
        monkeypatch.setenv(k, v)


def _why(c):
    return f"{c.name}: trace {FIXTURE[c.name]['trace']}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_single_frame_streams_and_fields(case, monkeypatch):
    """(a) ebcc_encode one frame: the reference build's stream (fixture; the live build where present), and ebcc_decode
    of it bit-equal to the oracle's decode."""
    _env(monkeypatch, case.quantile)
    x = case.field()
    want = FIXTURE[case.name]
    assert sha(x.tobytes()) == want["field_sha256"], case.name
    cfg = case.config(x)
    s = encode(x, cfg)
    assert len(s) == want["n"] and sha(s) == want["stream_sha256"], _why(case)
    if L.reference() is not None:
        assert s == L.ref_encode(x, cfg), _why(case)
    assert same_bits(decode(s), L.orc_decode(s)), _why(case)


def _groups():
    g = defaultdict(list)
    for c in CASES:
        g[(c.shape, c.quantile)].append(c)
    return sorted(g.items(), key=lambda kv: (kv[0][0], kv[0][1] or ""))


@pytest.mark.parametrize("group", _groups(), ids=lambda kv: f"{kv[0][0][0]}x{kv[0][0][1]}-q{kv[0][1] or 'default'}")
def test_batches_and_search_variants(group, monkeypatch):
    """(b) Context.encode_frames: every case of one shape and quantile with the fields of all the others in one batch
    under its config (their searches end in different rounds), and (c) the same batches under the search variants
    (short batches of rounds, one / three cut levels per round, no speculative rate allocation).  The case's
    own frame is the reference's stream, every other frame the product's single-frame stream of the same input, and
    Context.decode_frames gives the oracle's decode."""
    (shape, quantile), cases = group
    fields = [c.field() for c in cases]
    results = {}
    for extra in [{}] + VARIANTS:
        _env(monkeypatch, quantile, extra)
        with L.Context(len(cases), *shape) as ctx:
            for i, c in enumerate(cases):
                cfg = c.config(fields[i])
                # partners whose target would underflow to 0 under this config are left out (the reference asserts
                # error_target > 0 on them, :826)
                members = [k for k, other in enumerate(cases) if k == i or c.mode == L.NONE or
                           np.float32(cfg.error) * (np.float32(other.field().max()) - np.float32(other.field().min())
                                                    if c.mode == L.RELATIVE_ERROR else np.float32(1)) > 0]
                got = ctx.encode_frames(np.stack([fields[k] for k in members]), cfg)
                own = got[members.index(i)]
                assert sha(own) == FIXTURE[c.name]["stream_sha256"], (extra, _why(c))
                if not extra:
                    for k, s in zip(members, got):
                        assert s == encode(fields[k], cfg), (c.name, "partner", cases[k].name)
                    dec = ctx.decode_frames(got)
                    for k, s in enumerate(got):
                        assert same_bits(dec[k].ravel(), L.orc_decode(s)), (c.name, "decode", cases[members[k]].name)
                    results[c.name] = got
                else:
                    assert got == results[c.name], (extra, _why(c))


def test_bound_in_float64_without_mean_adjustment(monkeypatch):
    """EBCC_DISABLE_MEAN_ADJUSTMENT=1 (the adjustment, :864-868, may move the max error past the bound; the reference
    does that): the product's stream is the oracle's, and for every case whose search was feasible (fixture trace)
    max |decoded - original| <= bound in float64 numpy - the target, or relative x range - a check that rests on
    neither the oracle nor the product."""
    L.oracle().orc_set_j2k_backend(0)
    checked, bad = 0, []
    for c in CASES:
        _env(monkeypatch, c.quantile, {"EBCC_DISABLE_MEAN_ADJUSTMENT": "1"})
        x = c.field()
        cfg = c.config(x)
        s = encode(x, cfg)
        assert s == L.orc_encode(x, cfg), _why(c)
        if not feasible(FIXTURE[c.name]["trace"]):
            continue
        e = np.abs(decode(s).astype(np.float64) - x.ravel().astype(np.float64)).max()
        checked += 1
        if not e <= c.bound64(x):
            bad.append((c.name, float(e), c.bound64(x), FIXTURE[c.name]["trace"]))
    assert checked >= 40 and not bad, bad


def test_range_overflow_is_refused(monkeypatch):
    """max - min = inf (values at +-3e38): the reference build writes no stream (tests/test_search_branches.py), nor does
    the product - alone or in a batch."""
    _env(monkeypatch, None)
    c = D.overflow_case()
    assert FIXTURE[c.name]["refused"]
    x = c.field()
    cfg = c.config(x)
    assert encode(x, cfg) == b""
    lib = L.product()
    with L.Context(2, *c.shape) as ctx:
        frames = np.ascontiguousarray(np.stack([x, L.era5_like(*c.shape, 3)]), np.float32)
        d = L.DeviceArray(frames)
        outs = (ctypes.c_void_p * 2)()
        sizes = (ctypes.c_size_t * 2)()
        rc = lib.ebcc_hip_encode_frames(ctx.ptr, d.ptr, 2, ctypes.byref(cfg), outs, sizes)
        d.free()
        assert rc != 0 and not outs[0] and not outs[1]
        # the engine goes on working
        assert ctx.encode_frames(frames[1:], cfg)[0] == encode(frames[1], cfg)
