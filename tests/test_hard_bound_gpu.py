"""GPU: the hard-bound encode of include/ebcc_hip.h (ebcc_hip_encode_shard_hard / _host_frames_hard / _shard_groups_hard /
_host_frames_groups_hard).  The yardstick is the rule restated on the oracle (tests/_hard_bound.py: orc_ebcc_encode,
orc_ebcc_decode, float32 arithmetic): streams byte for byte, reports equal, and every final achieved <= target.

The three sets (era5_like(h, w, s, 1.0 + 0.1 * (s % 4), 0.6 + 0.3 * (s % 3))) and what the oracle's loop gives for them:
  max_64x96  64 x 96, seeds 0..15, MAX_ERROR 0.02, base_cr 20: seed 1 takes one re-encode, seed 3 two (its first re-encode gives
             the same 4948 bytes again), the others none
  max_40x50  40 x 50, seeds 0..11, MAX_ERROR 0.01, base_cr 10: seeds 0 and 10 miss (0.0123 against 0.01), one re-encode each
  rel_64x96  64 x 96, seeds 0..11, RELATIVE_ERROR 0.004, base_cr 20, EBCC_INIT_BASE_ERROR_QUANTILE=0.02 and the pure-base
             fallback disabled: 7 of 12 re-encoded, at most 2 rounds (seed 7 goes 0.247, 0.320, 0.105: not monotone)"""
import ctypes

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L

pytestmark = pytest.mark.gpu

BOUND_REPORT = np.dtype([("target", "<f4"), ("achieved", "<f4"), ("error_used", "<f4"), ("rounds", "<i4"), ("met", "<i4")])


class FrameGroup(ctypes.Structure):
    """ebcc_hip_frame_group"""
    _fields_ = [("frames", ctypes.c_void_p), ("n_frames", ctypes.c_size_t), ("config", L.CodecConfig), ("range_of_group", ctypes.c_int)]


def lib():
    """the product with the new entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    for name in ("ebcc_hip_encode_shard_hard", "ebcc_hip_encode_host_frames_hard"):
        fn = getattr(p, name)
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(L.CodecConfig), ctypes.c_int, L.c_void_pp, L.c_size_p,
                       ctypes.c_void_p]
        fn.restype = ctypes.c_int
    for name in ("ebcc_hip_encode_shard_groups_hard", "ebcc_hip_encode_host_frames_groups_hard"):
        fn = getattr(p, name)
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(FrameGroup), ctypes.c_size_t, ctypes.c_int, L.c_void_pp, L.c_size_p, ctypes.c_void_p]
        fn.restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


def take(outs, sizes, n):
    res = []
    for f in range(n):
        res.append(ctypes.string_at(outs[f], sizes[f]) if outs[f] else None)
        L.product().free_buffer(outs[f])
    return res


def encode_hard(x, cfg, cap, max_rounds=0, host=False):
    """-> (return value, streams, report) of the one-array entry points on a context of `cap` frames"""
    x = np.ascontiguousarray(x, np.float32)
    n, h, w = x.shape
    outs, sizes, report = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), np.zeros(n, BOUND_REPORT)
    with L.Context(cap, h, w) as ctx:
        if host:
            rc = lib().ebcc_hip_encode_host_frames_hard(ctx.ptr, x.ctypes.data, n, ctypes.byref(cfg), max_rounds, outs, sizes, report.ctypes.data)
        else:
            d = L.DeviceArray(x)
            rc = lib().ebcc_hip_encode_shard_hard(ctx.ptr, d.ptr, n, ctypes.byref(cfg), max_rounds, outs, sizes, report.ctypes.data)
            assert np.array_equal(d.get(np.float32, x.shape).view(np.uint32), x.view(np.uint32))          # (never written)
            d.free()
    return rc, take(outs, sizes, n), report


def want_report(loop):
    out = np.zeros(len(loop), BOUND_REPORT)
    for f, (_s, rep, _h) in enumerate(loop):
        out[f] = rep
    return out


def set_config(name):
    h, w, _n, mode, err, cr, _env = HB.SETS[name]
    return L.make_config((1, h, w), base_cr=cr, error=err, residual_type=mode)


ROUNDS = {"max_64x96": {1: 1, 3: 2}, "max_40x50": {0: 1, 10: 1}, "rel_64x96": {2: 1, 3: 2, 5: 1, 6: 1, 7: 2, 9: 1, 10: 1}}


@pytest.mark.parametrize("name", ["max_64x96", "max_40x50", "rel_64x96"])
def test_hard_against_the_rule_on_the_oracle(monkeypatch, name):
    HB.use_env(monkeypatch, HB.SETS[name][6])
    x, loop = HB.set_inputs(name), HB.set_loop(name)
    want = want_report(loop)
    n = len(x)
    assert {f: int(want["rounds"][f]) for f in range(n) if want["rounds"][f]} == ROUNDS[name]          # (what the oracle's loop is)
    assert (want["met"] == 1).all() and (want["achieved"] <= want["target"]).all()
    rc, streams, report = encode_hard(x, set_config(name), 16)
    print(name, "rounds", report["rounds"].tolist(), "achieved / target", (report["achieved"] / report["target"]).max())
    assert rc == 0, (L.product().ebcc_hip_last_error() or b"").decode()
    for f in range(n):
        assert streams[f] == loop[f][0], (name, f, len(streams[f]), len(loop[f][0]))
    assert report.tobytes() == want.tobytes(), (report, want)
    assert (report["achieved"] <= report["target"]).all() and (report["met"] == 1).all()
    # the frames that met the bound at once are those of the plain call, byte for byte
    with L.Context(16, x.shape[1], x.shape[2]) as ctx:
        plain = ctx.encode_frames(x, set_config(name))
    for f in range(n):
        assert (streams[f] == plain[f]) == (report["rounds"][f] == 0), (name, f)
    # the host form and a context of five frames (batches of 5 on the two engine sets): the same bytes
    for cap, host in ((16, True), (5, False), (5, True)):
        rc2, streams2, report2 = encode_hard(x, set_config(name), cap, host=host)
        assert rc2 == 0 and streams2 == streams and report2.tobytes() == report.tobytes(), (name, cap, host)


def test_one_round_is_not_enough_for_seed_3(monkeypatch):
    HB.use_env(monkeypatch, {})
    x, loop = HB.set_inputs("max_64x96"), HB.set_loop("max_64x96", 1)
    want = want_report(loop)
    assert want["met"].tolist() == [1, 1, 1, 0] + [1] * 12 and want["rounds"][3] == 1
    first = loop[3][2][0]                                       # (e_0, a_0, bytes) of seed 3: its re-encode is no better
    assert loop[3][2][1][1] >= first[1] and want["achieved"][3] == first[1] and want["error_used"][3] == np.float32(0.02)
    for host in (False, True):
        rc, streams, report = encode_hard(x, set_config("max_64x96"), 16, max_rounds=1, host=host)
        assert rc == 3
        assert all(streams[f] == loop[f][0] for f in range(16))
        assert report.tobytes() == want.tobytes(), (report, want)
        assert report["met"][3] == 0 and report["achieved"][3] > report["target"][3]
    # report may be NULL: the return value still says it
    n = 16
    outs, sizes = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)()
    with L.Context(16, 64, 96) as ctx:
        d = L.DeviceArray(np.ascontiguousarray(x))
        assert lib().ebcc_hip_encode_shard_hard(ctx.ptr, d.ptr, n, ctypes.byref(set_config("max_64x96")), 1, outs, sizes, None) == 3
        assert take(outs, sizes, n) == [s for s, _r, _h in loop]
        d.free()


def two_groups():
    """seeds 0..5 and 6..11 of the 64 x 96 set, the relative error of the second group, and the rule's loop for the twelve frames"""
    x = HB.set_inputs("max_64x96")
    g0, g1 = np.ascontiguousarray(x[:6]), np.ascontiguousarray(x[6:12])
    rel = np.float32(0.0005)
    restated = np.float32(rel * np.float32(g1.max() - g1.min()))

    def make():
        return [HB.harden(f, L.MAX_ERROR, 0.02, 20.0) for f in g0] + \
               [HB.harden(f, L.MAX_ERROR, float(restated), 20.0, target_value=restated) for f in g1]
    return g0, g1, rel, HB.once("two groups", make)


def test_two_groups_of_different_modes(monkeypatch):
    """G0: seeds 0..5 MAX_ERROR 0.02; G1: seeds 6..11 RELATIVE_ERROR 0.0005 of the range of the whole group, which the call restates
    as MAX_ERROR with error * (max - min) in float32 - the target the rule is then held against"""
    HB.use_env(monkeypatch, {})
    g0, g1, rel, loop = two_groups()
    want = want_report(loop)
    print("two groups: rounds", want["rounds"].tolist(), "targets", want["target"].tolist())
    assert want["rounds"][1] == 1 and want["rounds"][3] == 2 and (want["met"] == 1).all()
    seen = []
    for cap, host in ((16, False), (5, False), (5, True)):
        table = (FrameGroup * 2)()
        held = [g0, g1] if host else [L.DeviceArray(g0), L.DeviceArray(g1)]
        for g, (mode, err, whole) in enumerate(((L.MAX_ERROR, 0.02, 0), (L.RELATIVE_ERROR, float(rel), 1))):
            table[g].frames = held[g].ctypes.data if host else held[g].ptr
            table[g].n_frames = 6
            table[g].config = L.make_config((1, 64, 96), base_cr=20.0, error=err, residual_type=mode)
            table[g].range_of_group = whole
        outs, sizes, report = (ctypes.c_void_p * 12)(), (ctypes.c_size_t * 12)(), np.zeros(12, BOUND_REPORT)
        fn = lib().ebcc_hip_encode_host_frames_groups_hard if host else lib().ebcc_hip_encode_shard_groups_hard
        with L.Context(cap, 64, 96) as ctx:
            rc = fn(ctx.ptr, table, 2, 0, outs, sizes, report.ctypes.data)
        streams = take(outs, sizes, 12)
        assert rc == 0, (cap, host, (L.product().ebcc_hip_last_error() or b"").decode())
        assert streams == [s for s, _r, _h in loop], (cap, host)
        assert report.tobytes() == want.tobytes(), (cap, host, report, want)
        seen.append(streams)
    assert seen[0] == seen[1] == seen[2]


def test_none_mode_and_constant_frames_are_left_alone(monkeypatch):
    HB.use_env(monkeypatch, {})
    x = np.array(HB.set_inputs("max_64x96")[:4])
    x[2] = 3.25
    cfg = L.make_config((1, 64, 96), base_cr=20.0, error=0.0, residual_type=L.NONE)
    rc, streams, report = encode_hard(x, cfg, 16)
    assert rc == 0 and (report["rounds"] == 0).all() and (report["met"] == 1).all() and np.isinf(report["target"]).all()
    with L.Context(16, 64, 96) as ctx:
        assert streams == ctx.encode_frames(x, cfg)
    cfg = set_config("max_64x96")
    rc, streams, report = encode_hard(x, cfg, 16)
    assert rc == 0 and report["rounds"].tolist() == [0, 1, 0, 2] and report["achieved"][2] == 0 and report["met"][2] == 1


def test_failures_free_every_stream():
    x = np.array(HB.set_inputs("max_64x96")[:6])
    x[4, 3, 3] = np.nan
    for host in (False, True):
        rc, streams, _report = encode_hard(x, set_config("max_64x96"), 4, host=host)
        assert rc == 2 and streams == [None] * 6


def test_python_batch_codec(monkeypatch):
    """ebcc_amd/h5_batch.py: BatchCodec.encode(hard=True), encode_groups(hard=True) and audit, on an engine of five frames"""
    from ebcc_amd import h5_batch
    HB.use_env(monkeypatch, {})
    x, loop = HB.set_inputs("max_64x96"), HB.set_loop("max_64x96")
    cfg = h5_batch.frame_config(64, 96, 20.0, ("max_error_target", 0.02))
    with h5_batch.BatchCodec(64, 96, max_frames=5) as codec:
        streams, report = codec.encode(x, cfg, hard=True)
        assert streams == [s for s, _r, _h in loop] and report.tobytes() == want_report(loop).tobytes()
        audit = codec.audit(streams, x, bound=0.02)
        assert (audit["n_over"] == 0).all() and audit["max_abs"].tobytes() == report["achieved"].tobytes()
        soft = codec.encode(x, cfg)
        assert np.flatnonzero(codec.audit(soft, x, bound=np.full(16, 0.02, np.float32))["n_over"]).tolist() == [1, 3]
        _streams, short = codec.encode(x, cfg, hard=True, max_rounds=1)
        assert short["met"].tolist() == [1, 1, 1, 0] + [1] * 12
        g0, g1, rel, both = two_groups()
        coded, rep = codec.encode_groups([(g0, 20.0, ("max_error_target", 0.02)), (g1, 20.0, ("relative_error_target", float(rel)), True)], hard=True)
        assert coded[0] + coded[1] == [s for s, _r, _h in both] and rep.tobytes() == want_report(both).tobytes()
        with pytest.raises(ValueError):
            bad = np.array(x)
            bad[0, 0, 0] = np.inf
            codec.audit(streams, bad)
