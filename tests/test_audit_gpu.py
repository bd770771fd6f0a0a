"""GPU: the audit of include/ebcc_hip.h - ebcc_hip_frame_errors (k_frame_errors alone) against numpy, and ebcc_hip_audit_frames /
_shard / _host_frames against the same statistics taken with numpy on the oracle's decode of the same streams.

Exact: max_abs, at (first occurrence), n_over, x_min, x_max.  The sums in double are compared within n * 2^-52 * sum |term|, the
worst case of n double additions in any order (each addition errs by at most 2^-53 of a partial sum, which is at most
sum |term|; numpy's own pairwise sum is inside the same bound, hence 2^-52 for the two together) - derived, not measured."""
import ctypes

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L

pytestmark = pytest.mark.gpu

FRAME_ERROR = np.dtype([("max_abs", "<f4"), ("at", "<u4"), ("n_over", "<u8"), ("sum", "<f8"), ("sum_sq", "<f8"), ("x_min", "<f4"), ("x_max", "<f4")])
SENT = np.uint32(0xA5A5A5A5)
FRONT, BACK = 64, 37                                  # floats of sentinel before (256 bytes) and behind
H, W = 64, 96


def lib():
    """the product with the audit entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    p.ebcc_hip_frame_errors.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                        ctypes.c_void_p, ctypes.c_void_p]
    for name in ("ebcc_hip_audit_frames", "ebcc_hip_audit_shard", "ebcc_hip_audit_host_frames"):
        fn = getattr(p, name)
        fn.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        fn.restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


class Resident:
    """a host array on the device, beginning `base` floats behind a 256-byte boundary, sentinels around it"""

    def __init__(self, host, base):
        host = np.ascontiguousarray(host, np.float32)
        self.words = np.concatenate([np.full(FRONT + base, SENT, np.uint32), host.view(np.uint32).ravel(), np.full(BACK, SENT, np.uint32)])
        self.d = L.DeviceArray(self.words)
        assert self.d.ptr % 256 == 0
        self.ptr = self.d.ptr + 4 * (FRONT + base)

    def untouched(self):
        return np.array_equal(self.d.get(np.uint32, self.words.shape), self.words)


def numpy_report(x, d, bound=None):
    out = np.zeros(len(x), FRAME_ERROR)
    for f in range(len(x)):
        out[f] = HB.stats(x[f], d[f], None if bound is None else bound[f])
    return out


def check(got, want, x, d, what):
    for name in ("max_abs", "at", "n_over", "x_min", "x_max"):
        assert got[name].tobytes() == want[name].tobytes(), (what, name, got[name], want[name])
    for f in range(len(x)):
        e = x[f].astype(np.float64).ravel() - d[f].astype(np.float64).ravel()
        n = e.size
        print(what, f, "sum", got["sum"][f] - want["sum"][f], "of", n * 2.0 ** -52 * np.abs(e).sum(),
              "sum_sq", got["sum_sq"][f] - want["sum_sq"][f], "of", n * 2.0 ** -52 * (e * e).sum())
        assert abs(got["sum"][f] - want["sum"][f]) <= n * 2.0 ** -52 * np.abs(e).sum(), (what, f)
        assert abs(got["sum_sq"][f] - want["sum_sq"][f]) <= n * 2.0 ** -52 * (e * e).sum(), (what, f)


# ---- the kernel alone --------------------------------------------------------------------------------------------------------
def kernel_case(h, w):
    """three frames and what was decoded of them: frame 0 with the largest error planted twice, frame 1 with -0 as its minimum,
    frame 2 with -0 as its maximum"""
    r = np.random.default_rng(h * 1000 + w)
    x = (r.standard_normal((3, h, w)) * 3 + 5).astype(np.float32)
    x[1] = np.abs(x[1])
    x[2] = -np.abs(x[2])
    x[1, h // 2, w // 3] = -0.0
    x[2, h // 3, w // 2] = -0.0
    d = (x + r.standard_normal(x.shape).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    for y, c in ((h - 2, w - 3), (h // 2, 5)):                    # (the later pixel first: the earlier one must win)
        x[0, y, c], d[0, y, c] = 2.0, 1.0
    return x, d, np.array([0.01, 0.02, 0.005], np.float32)


@pytest.mark.parametrize("h,w", [(37, 53), (64, 96), (90, 131)])      # (one workgroup a frame with and without a tail; two)
@pytest.mark.parametrize("bases", [(1, 0), (0, 1)])
def test_kernel_against_numpy(h, w, bases):
    x, d, bound = kernel_case(h, w)
    want = numpy_report(x, d, bound)
    assert want["at"][0] == (h // 2) * w + 5 and want["max_abs"][0] == 1.0
    assert want["x_min"][1].tobytes() == np.float32(0.0).tobytes() and want["x_max"][2].tobytes() == np.float32(0.0).tobytes()
    assert (want["n_over"] > 0).all()
    with L.Context(4, 64, 96) as ctx:                            # (any context of the device)
        rx, rd = Resident(x, bases[0]), Resident(d, bases[1])
        got = np.zeros(3, FRAME_ERROR)
        assert lib().ebcc_hip_frame_errors(ctx.ptr, rx.ptr, rd.ptr, 3, h, w, bound.ctypes.data, got.ctypes.data) == 0
        check(got, want, x, d, f"{h}x{w} {bases}")
        again = np.zeros(3, FRAME_ERROR)
        assert lib().ebcc_hip_frame_errors(ctx.ptr, rx.ptr, rd.ptr, 3, h, w, bound.ctypes.data, again.ctypes.data) == 0
        assert again.tobytes() == got.tobytes()
        # without bounds nothing is counted; the rest is the same
        free = np.zeros(3, FRAME_ERROR)
        assert lib().ebcc_hip_frame_errors(ctx.ptr, rx.ptr, rd.ptr, 3, h, w, None, free.ctypes.data) == 0
        assert (free["n_over"] == 0).all()
        free["n_over"] = got["n_over"]
        assert free.tobytes() == got.tobytes()
        assert rx.untouched() and rd.untouched()


def test_kernel_sums_do_not_depend_on_alignment():
    x, d, bound = kernel_case(37, 53)
    with L.Context(4, 64, 96) as ctx:
        seen = set()
        for bx in range(4):
            for bd in range(4):
                rx, rd = Resident(x, bx), Resident(d, bd)
                got = np.zeros(3, FRAME_ERROR)
                assert lib().ebcc_hip_frame_errors(ctx.ptr, rx.ptr, rd.ptr, 3, 37, 53, bound.ctypes.data, got.ctypes.data) == 0
                seen.add(got.tobytes())
        assert len(seen) == 1


def test_kernel_nan_in_originals():
    x, d, _ = kernel_case(37, 53)
    x[1, 36, 52] = np.nan                                        # (the frame's last pixel: the tail)
    with L.Context(4, 64, 96) as ctx:
        rx, rd = Resident(x, 1), Resident(d, 0)
        got = np.zeros(3, FRAME_ERROR)
        assert lib().ebcc_hip_frame_errors(ctx.ptr, rx.ptr, rd.ptr, 3, 37, 53, None, got.ctypes.data) == 2
        want = numpy_report(x[[0, 2]], d[[0, 2]])                        # (the frames without one are still reported)
        for name in ("max_abs", "at", "n_over", "x_min", "x_max"):
            assert got[[0, 2]][name].tobytes() == want[name].tobytes(), name
        x[1, 36, 52] = np.inf
        rx = Resident(x, 1)
        assert lib().ebcc_hip_frame_errors(ctx.ptr, rx.ptr, rd.ptr, 3, 37, 53, None, got.ctypes.data) == 2
        assert rx.untouched() and rd.untouched()


# ---- the audit entry points against the oracle ---------------------------------------------------------------------------------
def mixed_batch():
    """eleven frames of 64 x 96, their streams from the oracle, and numpy's statistics on the oracle's decode of them:
    0-3 MAX_ERROR 0.02 (1 and 3 miss it), 4-5 RELATIVE_ERROR 0.004, 6 NONE, 7 constant, 8 a legacy header-less stream, 9-10 MAX_ERROR"""
    def make():
        L.oracle().orc_set_j2k_backend(0)
        x = np.array(HB.set_inputs("max_64x96")[:11])
        x[7] = 7.0
        cfg = lambda mode, err: L.make_config((1, H, W), base_cr=20.0, error=err, residual_type=mode)      # noqa: E731
        modes = [L.MAX_ERROR] * 4 + [L.RELATIVE_ERROR] * 2 + [L.NONE] + [L.MAX_ERROR] * 4
        errs = [0.02] * 4 + [0.004] * 2 + [0.0] + [0.02] * 4
        streams = [L.orc_encode(x[f], cfg(modes[f], errs[f])) for f in range(11)]
        assert all(streams)
        decoded = np.stack([L.orc_decode(s).reshape(H, W) for s in streams])
        streams[8] = L.legacy_repack(streams[8])
        bound = np.array([float(HB.target(x[f], modes[f], errs[f])) if modes[f] else 1e30 for f in range(11)], np.float32)
        want = numpy_report(x, decoded, bound)
        assert want["max_abs"][7] == 0 and want["n_over"][1] > 0 and want["n_over"][3] > 0
        x.setflags(write=False)
        return x, streams, decoded, bound, want
    return HB.once("audit mixed batch", make)


def run_audit(form, cap, x, streams, bound):
    n = len(streams)
    bufs = [ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p).value for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    got = np.zeros(n, FRAME_ERROR)
    with L.Context(cap, H, W) as ctx:
        if form == "host":
            host = np.concatenate([np.full(3, 9e9, np.float32), x.ravel(), np.full(5, 9e9, np.float32)])     # (4-byte aligned only)
            keep = host.copy()
            rc = lib().ebcc_hip_audit_host_frames(ctx.ptr, ptrs, sizes, n, host[3:].ctypes.data, bound.ctypes.data, got.ctypes.data)
            assert host.tobytes() == keep.tobytes()
        else:
            rx = Resident(x, 1)
            fn = lib().ebcc_hip_audit_frames if form == "frames" else lib().ebcc_hip_audit_shard
            rc = fn(ctx.ptr, ptrs, sizes, n, rx.ptr, bound.ctypes.data, got.ctypes.data)
            assert rx.untouched()
    return rc, got


def test_audit_against_oracle(monkeypatch):
    HB.use_env(monkeypatch, {})
    x, streams, decoded, bound, want = mixed_batch()
    seen = {}
    for form, cap in (("frames", 16), ("shard", 16), ("shard", 5), ("host", 16), ("host", 5)):
        rc, got = run_audit(form, cap, x, streams, bound)
        assert rc == 0, (form, cap, (L.product().ebcc_hip_last_error() or b"").decode())
        check(got, want, x, decoded, f"{form} capacity {cap}")
        seen[(form, cap)] = got.tobytes()
    assert len(set(seen.values())) == 1, [k for k, v in seen.items() if v != seen[("frames", 16)]]
    rc, again = run_audit("shard", 5, x, streams, bound)
    assert rc == 0 and again.tobytes() == seen[("shard", 5)]


def test_audit_refuses_as_the_decode_does(monkeypatch):
    HB.use_env(monkeypatch, {})
    x, streams, _decoded, bound, _want = mixed_batch()
    rc, _ = run_audit("frames", 5, x, streams, bound)                   # (more frames than the context holds)
    assert rc == 1
    bad = list(streams)
    bad[2] = bad[2][:40]
    for form in ("shard", "host"):
        rc, _ = run_audit(form, 16, x, bad, bound)
        assert rc == 1, form
    nan = np.array(x)
    nan[9, 5, 5] = np.nan
    for form in ("shard", "host"):
        rc, got = run_audit(form, 5, nan, streams, bound)
        assert rc == 2, form


def test_audit_finds_the_frames_over_the_bound(monkeypatch):
    """the 64 x 96 MAX_ERROR 0.02 set: seeds 1 and 3 miss the bound, on the oracle and here"""
    HB.use_env(monkeypatch, {})
    x = HB.set_inputs("max_64x96")
    loop = HB.set_loop("max_64x96")
    cfg = L.make_config((1, H, W), base_cr=20.0, error=0.02, residual_type=L.MAX_ERROR)
    plain = HB.once("plain max_64x96", lambda: [L.orc_encode(f, cfg) for f in x])
    over = [s for s in range(16) if HB.stats(x[s], L.orc_decode(plain[s]), 0.02)[2] > 0]
    assert over == [1, 3] and [s for s in range(16) if loop[s][1][3] > 0] == [1, 3]
    bound = np.full(16, 0.02, np.float32)
    rc, got = run_audit("shard", 16, x, plain, bound)
    assert rc == 0
    assert [s for s in range(16) if got["n_over"][s] > 0] == [1, 3]
    assert [s for s in range(16) if got["max_abs"][s] > np.float32(0.02)] == [1, 3]
