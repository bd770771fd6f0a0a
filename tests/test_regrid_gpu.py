"""GPU: the regrid decode of include/ebcc_hip.h - ebcc_hip_regrid_items (k_regrid alone) on numpy's own arrays, and
ebcc_hip_regrid_shard / ebcc_hip_regrid_host_frames on streams, against the numpy restatement of the header's rule
(tests/_regrid.py) applied to the arrays or to the oracle's decode of the same streams - never to the product's decode.
Everything is compared by tobytes(): there is no tolerance in this file.

The order of the taps is visible only where a support cancels (tests/_regrid.py: items): the tests of the kernel that rely on it
- block means of 4 and 7, the pixel of 256 x 256 taps, the wrapping map - first assert that their expected bytes differ from
float32 accumulation and from the taps in reverse.  The tests on streams do not rely on it: a lossy decode keeps no exact
cancellation, and what they check is the plumbing - boxes, batches, engine sets, offsets.

The identity: by the rule a sample of -0 leaves as +0 (t = +0.0 + (-0.0) * 1.0), so the identity returns the bytes of x + 0.0f;
on items without a -0 those are the input's own bytes, and both are asserted.

Not tested here: the refusal of a context for chunks of several frames - the C interface has no call that makes one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ebcc_amd import regrid as M
from tests import _hard_bound as HB
from tests import _lib as L
from tests import _regrid as R
from tests import test_reduce_gpu as RG
from tests import test_window_gpu as T

pytestmark = pytest.mark.gpu

Guarded = RG.Guarded
last_error = RG.last_error
JUNK = np.float32(-7.5e9)                                # what `out` holds before a call


def lib():
    """the product with the regrid entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    p.ebcc_hip_regrid_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                        ctypes.POINTER(R.RegridSpec), ctypes.c_void_p]
    for name in ("ebcc_hip_regrid_shard", "ebcc_hip_regrid_host_frames"):
        getattr(p, name).argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.POINTER(R.RegridSpec), ctypes.c_void_p]
    p.ebcc_hip_decode_frames.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p]
    for name in ("ebcc_hip_regrid_items", "ebcc_hip_regrid_shard", "ebcc_hip_regrid_host_frames", "ebcc_hip_decode_frames"):
        getattr(p, name).restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


def device_out(n, rows, cols, base=0):
    return Guarded(np.full((n, rows.n_out, cols.n_out), JUNK, np.float32), base)


def regrid_items(ctx, items, rows, cols, out=None, base=0):
    """ebcc_hip_regrid_items of the Guarded items [n][h][w] -> (status, Guarded output)"""
    n, h, w = items.shape
    out = out or device_out(n, rows, cols, base)
    spec = M.regrid_spec(rows, cols)
    return lib().ebcc_hip_regrid_items(ctx.ptr, items.ptr, n, h, w, ctypes.byref(spec), out.ptr), out


# ---- 1. the kernel alone against numpy -----------------------------------------------------------------------------------
GEOMETRIES = [(5, 777), (130, 9), (37, 70)]


def uneven(n, k):
    """a conservative map of n cells onto k cells whose edges fall on no source edge"""
    return M.conservative_map(np.arange(n + 1.0), np.linspace(0.3, n - 0.4, k + 1))


def difference(n):
    """(x[i + 2] - x[i]) / 2: negative weights, and a tap of weight 0 between them"""
    return M.AxisMap(np.arange(n - 2), np.full(n - 2, 3), np.tile([-0.5, 0.0, 0.5], n - 2))


def seam(w):
    """supports of five taps with 1, 2 and 4 (count - 1) of them beyond the seam, one that ends on the last column, one inside"""
    return M.AxisMap([w - 4, w - 3, w - 1, w - 5, 1], [5] * 5, np.tile([1.0, 1.0, 1.0, 0.5, -0.25], 5), wrap=True)


def kernel_maps(h, w):
    """{name: (row map, column map, the order must be visible)}"""
    maps = {"identity": (M.identity_map(h), M.identity_map(w), False), "flip": (M.flip_map(h), M.flip_map(w), False),
            "flip rows": (M.flip_map(h), M.identity_map(w), False)}
    for k in (2, 3, 4, 7):
        maps[f"mean {k}"] = (M.block_mean_map(h, k), M.block_mean_map(w, k), k in (4, 7))
    maps["mean 4 of weighted rows"] = (M.block_mean_map(h, 4, weights=np.cos(np.linspace(-1.5, 1.5, h))), M.block_mean_map(w, 3), False)
    maps["conservative"] = (uneven(h, {5: 2, 130: 17, 37: 5}[h]), uneven(w, {777: 100, 9: 4, 70: 9}[w]), False)
    maps["linear up"] = (M.linear_map(np.arange(h), np.linspace(0, h - 1, h + h // 2 + 3)), M.linear_map(np.arange(w), np.linspace(0, w - 1, 2 * w + 7)), False)
    maps["seam"] = (M.block_mean_map(h, 4), seam(w), True)
    maps["difference"] = (difference(h), difference(w), False)
    return maps


@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_kernel_against_numpy(h, w):
    x = R.items(h, w)
    if (h, w) == (130, 9):
        lin = kernel_maps(h, w)["linear up"][1]
        assert lin.n_out == 25 and lin.n_out > w                     # 9 -> 25 columns: the output is larger than the input
    with L.Context(4, 64, 96) as ctx:                                # (any context of the device)
        items = Guarded(x, 1)
        for name, (rows, cols, visible) in kernel_maps(h, w).items():
            if visible:
                assert R.order_is_visible(x, rows, cols), name
            want = R.apply(x, rows, cols)
            rc, out = regrid_items(ctx, items, rows, cols, base=3)
            assert rc == 0, (name, last_error())
            assert out.get().tobytes() == want.tobytes(), (h, w, name)
            assert out.sentinels_intact() and items.untouched(), name
        # the identity: -0 leaves as +0, everything else as it came
        rc, out = regrid_items(ctx, items, M.identity_map(h), M.identity_map(w))
        assert rc == 0 and out.get().tobytes() == (x + np.float32(0.0)).tobytes() != x.tobytes()
        plain = np.where(x == 0, np.float32(0.0), x)
        rc, out = regrid_items(ctx, Guarded(plain, 2), M.identity_map(h), M.identity_map(w))
        assert rc == 0 and out.get().tobytes() == plain.tobytes()
        rc, out = regrid_items(ctx, Guarded(plain, 2), M.flip_map(h), M.flip_map(w))
        assert rc == 0 and out.get().tobytes() == plain[:, ::-1, ::-1].tobytes()
        # a second run: the same bytes
        rows, cols, _ = kernel_maps(h, w)["mean 7"]
        first = regrid_items(ctx, items, rows, cols)[1].get().tobytes()
        assert regrid_items(ctx, items, rows, cols)[1].get().tobytes() == first


def test_one_pixel_of_256_x_256_taps():
    """the longest supports the interface takes, on both axes at once, with weights of both signs; and every count from 1 to 9
    around the kernel's two paths (column supports of up to eight taps are kept in registers), and supports of twelve taps
    with 11, 1 and 6 of them beyond the seam"""
    h, w = 256, 300
    x = R.items(h, w)
    r = np.random.default_rng(9)
    ones = (M.AxisMap([0], [256], np.ones(256)), M.AxisMap([44], [256], np.ones(256)))
    mixed = (M.AxisMap([0], [256], r.standard_normal(256)), M.AxisMap([44], [256], r.standard_normal(256)))
    assert R.order_is_visible(x, *ones)
    counts = np.arange(1, 10)
    ladder = [M.AxisMap(np.arange(9) * 20, counts, r.standard_normal(counts.sum())), M.AxisMap(np.arange(9) * 30 + 3, counts, np.ones(counts.sum()))]
    short = [M.AxisMap(np.arange(8) * 20, counts[:8], r.standard_normal(36)), M.AxisMap(np.arange(8) * 32, counts[:8], np.ones(36))]
    assert R.order_is_visible(x, *short)
    long_seam = (M.block_mean_map(h, 7), M.AxisMap([w - 1, w - 11, w - 6, 150], [12] * 4, np.tile([1.0] * 10 + [0.5, -0.25], 4), wrap=True))
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 2)
        for name, (rows, cols) in (("ones", ones), ("mixed", mixed), ("counts 1 .. 9", ladder), ("counts 1 .. 8", short),
                                   ("twelve taps across the seam", long_seam)):
            rc, out = regrid_items(ctx, items, rows, cols, base=1)
            assert rc == 0, last_error()
            assert out.get().tobytes() == R.apply(x, rows, cols).tobytes(), name
            assert out.sentinels_intact() and items.untouched()


def test_results_do_not_depend_on_alignment():
    h, w = 37, 70
    x = R.items(h, w)
    seen = set()
    with L.Context(4, 64, 96) as ctx:
        for name in ("mean 7", "seam", "conservative"):
            rows, cols, _ = kernel_maps(h, w)[name]
            want = R.apply(x, rows, cols).tobytes()
            for item_base in range(4):
                items = Guarded(x, item_base)
                for out_base in range(4):
                    rc, out = regrid_items(ctx, items, rows, cols, base=out_base)
                    assert rc == 0, last_error()
                    assert out.get().tobytes() == want and out.sentinels_intact(), (name, item_base, out_base)
                    seen.add(out.get().tobytes())
    assert len(seen) == 3


def test_refused_calls_write_nothing():
    h, w = 37, 70
    x = R.items(h, w)
    rows, cols, _ = kernel_maps(h, w)["mean 4"]
    spec = M.regrid_spec(rows, cols)
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 0)
        out = device_out(3, rows, cols)
        f = lib().ebcc_hip_regrid_items
        assert f(ctx.ptr, items.ptr + 2, 3, h, w, ctypes.byref(spec), out.ptr) == 1 and last_error()     # items not 4-byte aligned
        assert f(ctx.ptr, items.ptr, 3, h, w, ctypes.byref(spec), out.ptr + 1) == 1 and last_error()     # nor the output
        assert f(ctx.ptr, None, 3, h, w, ctypes.byref(spec), out.ptr) == 1
        assert f(ctx.ptr, items.ptr, 3, h, w, ctypes.byref(spec), None) == 1
        assert f(ctx.ptr, items.ptr, 0, h, w, ctypes.byref(spec), out.ptr) == 1
        assert f(ctx.ptr, items.ptr, 3, h, w, None, out.ptr) == 1
        assert f(None, items.ptr, 3, h, w, ctypes.byref(spec), out.ptr) == 1
        assert f(ctx.ptr, items.ptr, 3, h - 1, w, ctypes.byref(spec), out.ptr) == 1 and "row output" in last_error()   # the map leaves the items
        assert f(ctx.ptr, items.ptr, 3, h, w - 1, ctypes.byref(spec), out.ptr) == 1 and "column output" in last_error()
        bad = M.AxisMap([0], [2], [1.0, 2.0])
        bad.weight[1] = np.nan
        rc, out2 = regrid_items(ctx, items, rows, bad, out=out)
        assert rc == 1 and "NaN" in last_error()
        rc, out2 = regrid_items(ctx, items, M.AxisMap([0], [1], [1.0], wrap=True), cols, out=out)
        assert rc == 1 and "wrap" in last_error()
        assert out.untouched() and items.untouched()
        rc, out = regrid_items(ctx, items, rows, cols, out=out)        # and the context still works
        assert rc == 0 and out.get().tobytes() == R.apply(x, rows, cols).tobytes()


def test_launch_limits():
    """The launches of regrid_items are cut by one count: the item is blockIdx.z, so a launch takes at most 65535 items.  70 000
    items of 2 x 4 onto one pixel each run as two launches.  Nothing else is cut: gridDim.y is the output row (n_out <= 65535 by
    the check) and gridDim.x the runs of 256 output columns (at most 256)."""
    n, h, w = 70000, 2, 4
    r = np.random.default_rng(7)
    x = (r.standard_normal((n, h, w)) * 3 + 5).astype(np.float32) * np.asarray(R.SCALES, np.float32)[np.arange(w) % 3][None, None, :]
    x[1::2, :, 0] = np.float32(4e6)
    x[1::2, :, 2] = np.float32(-4e6)                                  # (odd items cancel: the order shows)
    rows, cols = M.AxisMap([0], [2], [0.75, 1.0 / 3.0]), M.AxisMap([0], [4], [1.0, 1.0, 1.0, 0.5])
    assert n > 65535 and R.order_is_visible(x, rows, cols)
    want = R.apply(x, rows, cols)
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 1)
        rc, out = regrid_items(ctx, items, rows, cols, base=1)
        assert rc == 0, last_error()
        got = out.get()
        assert got[:65535].tobytes() == want[:65535].tobytes() and got[65535:].tobytes() == want[65535:].tobytes()
        assert out.sentinels_intact() and items.untouched()


# ---- 2. streams against the oracle, across batches -------------------------------------------------------------------------
H, W = RG.H, RG.W
N = 37


def catalogue():
    """37 streams of 64 x 96 and the oracle's decode of each: the twelve of the reduce tests (base layer and residual layer)
    in turn, with a constant field, a frame without a residual layer and a legacy header-less stream among them"""
    streams, fields = RG.series(H, W, 12)

    def make():
        x = np.stack([np.full((H, W), 7.25e6, np.float32), HB.inputs(H, W, [20])[0]])
        with L.Context(4, H, W) as ctx:
            const = ctx.encode_frames(x[:1], L.make_config((1, H, W), base_cr=20.0, error=0.004, residual_type=L.RELATIVE_ERROR))[0]
            base_only = ctx.encode_frames(x[1:], L.make_config((1, H, W), base_cr=20.0, error=0.0, residual_type=L.NONE))[0]
        mixed = [streams[i % 12] for i in range(N)]
        mixed[5], mixed[17], mixed[30], mixed[36] = const, L.legacy_repack(streams[1]), base_only, const
        L.oracle().orc_set_j2k_backend(0)
        known = {}
        for s in mixed:
            if s not in known:
                known[s] = L.orc_decode(s).reshape(H, W)
        decoded = np.stack([known[s] for s in mixed])
        decoded.setflags(write=False)
        return mixed, decoded
    return HB.once("regrid catalogue", make)


def stream_maps():
    """{name: (row map, column map)}: the whole frame, a window, and a wrapping map over bounded rows"""
    window = (M.conservative_map(np.arange(H + 1.0), np.linspace(10.0, 50.0, 8)), M.conservative_map(np.arange(W + 1.0), np.linspace(20.0, 70.0, 12)))
    assert R.bounding(*window, H, W) == (10, 20, 40, 50)
    wrapping = (M.AxisMap([12, 15, 21], [3, 6, 3], np.full(12, 0.25)), seam(W))
    assert R.bounding(*wrapping, H, W) == (12, 0, 12, W)
    return {"mean 4 x 4": (M.block_mean_map(H, 4), M.block_mean_map(W, 4)), "window": window, "wrapping": wrapping}


def regrid_streams(ctx, streams, rows, cols, host=False, base=0, out=None):
    """ebcc_hip_regrid_shard (-> Guarded) or ebcc_hip_regrid_host_frames (-> a numpy array between margins) -> (status, out)"""
    keep, ptrs, sizes = RG._args(streams)
    spec = M.regrid_spec(rows, cols)
    n = len(streams)
    if host:
        out = out if out is not None else HostOut(n, rows, cols, base)
        return lib().ebcc_hip_regrid_host_frames(ctx.ptr, ptrs, sizes, n, ctypes.byref(spec), out.ptr), out
    out = out or device_out(n, rows, cols, base)
    return lib().ebcc_hip_regrid_shard(ctx.ptr, ptrs, sizes, n, ctypes.byref(spec), out.ptr), out


class HostOut:
    """the host output [n][Ro][Co] between margins of junk, `base` words behind the start of its array"""
    MARGIN = 16

    def __init__(self, n, rows, cols, base=0):
        self.shape = (n, rows.n_out, cols.n_out)
        size = n * rows.n_out * cols.n_out
        self.buf = np.full(size + 2 * self.MARGIN + 4, JUNK, np.float32)
        self.lo = self.MARGIN + base
        self.body = self.buf[self.lo:self.lo + size]

    @property
    def ptr(self):
        return self.body.ctypes.data

    def get(self):
        return self.body.reshape(self.shape).copy()

    def sentinels_intact(self):
        return bool((self.buf[:self.lo].view(np.uint32) == JUNK.view(np.uint32)).all() and
                    (self.buf[self.lo + self.body.size:].view(np.uint32) == JUNK.view(np.uint32)).all())

    def untouched(self):
        return bool((self.buf.view(np.uint32) == JUNK.view(np.uint32)).all())


def test_streams_against_the_oracle_across_batches(monkeypatch):
    """capacity 5: eight batches on the two engine sets, the last of two frames; 16: three batches, the last of five; 64: one"""
    HB.use_env(monkeypatch, {})
    streams, fields = catalogue()
    maps = stream_maps()
    want = {name: R.apply(fields, *m).tobytes() for name, m in maps.items()}
    seen = {name: [] for name in maps}
    for cap in (5, 16, 64):
        with L.Context(cap, H, W) as ctx:
            for name, (rows, cols) in maps.items():
                rc, out = regrid_streams(ctx, streams, rows, cols, base=cap % 4)
                assert rc == 0, (name, cap, last_error())
                assert out.get().tobytes() == want[name], (name, cap)
                assert out.sentinels_intact()
                rc, host = regrid_streams(ctx, streams, rows, cols, host=True, base=(cap + 1) % 4)
                assert rc == 0, (name, cap, last_error())
                assert host.get().tobytes() == out.get().tobytes() and host.sentinels_intact(), (name, cap)
                seen[name].append(out.get().tobytes())
    for name in maps:
        assert seen[name][0] == seen[name][1] == seen[name][2]


def test_a_box_gives_the_bytes_of_the_frame(monkeypatch):
    """the window map and the wrapping map, decoded as their boxes, against the same maps applied by ebcc_hip_regrid_items to
    what ebcc_hip_decode_shard returns; and the output at every word offset"""
    HB.use_env(monkeypatch, {})
    streams, fields = catalogue()
    maps = stream_maps()
    with L.Context(16, H, W) as ctx:
        decoded = ctx.decode_frames(streams, shard=True)
        assert np.array_equal(decoded, fields)
        frames = Guarded(decoded, 1)
        for name in ("window", "wrapping"):
            rows, cols = maps[name]
            rc, whole = regrid_items(ctx, frames, rows, cols)
            assert rc == 0, last_error()
            for base in range(4):
                rc, out = regrid_streams(ctx, streams, rows, cols, base=base)
                assert rc == 0, last_error()
                assert out.get().tobytes() == whole.get().tobytes() and out.sentinels_intact(), (name, base)
                rc, host = regrid_streams(ctx, streams, rows, cols, host=True, base=base)
                assert rc == 0 and host.get().tobytes() == whole.get().tobytes() and host.sentinels_intact(), (name, base)


# ---- 3. refusals on the device ---------------------------------------------------------------------------------------------
def test_refusals_and_a_stream_damaged_inside_a_batch(monkeypatch):
    """What is refused before anything is written - with a message that names the frame where a frame is at fault -, and the
    damaged stream of tests/test_codec_gpu.py::test_malformed_streams_are_rejected (a frame without a residual layer cut to 40
    bytes: its frame header parses, the decode of its batch refuses it) in the first batch and in the last: the call returns
    what ebcc_hip_decode_frames returns for the same bytes, nothing outside `out` is written, and the next call is correct."""
    HB.use_env(monkeypatch, {})
    streams, fields = catalogue()
    rows, cols = stream_maps()["window"]
    want = R.apply(fields, rows, cols).tobytes()

    def make():
        with L.Context(4, H, W) as ctx:
            return ctx.encode_frames(L.era5_like(H, W, 64)[None], L.make_config((1, H, W), base_cr=10, residual_type=L.NONE))[0][:40]
    damaged = HB.once("reduce damaged stream", make)
    with L.Context(5, 90, 131) as other:                            # a context of another geometry
        for host in (False, True):
            rc, out = regrid_streams(other, streams, rows, cols, host=host)
            assert rc == 1 and last_error() and out.sentinels_intact()
            rc, out = regrid_streams(other, streams, M.identity_map(H), M.identity_map(W), host=host)      # (the whole frame of the streams)
            assert rc == 1 and last_error() and out.sentinels_intact()
    with L.Context(5, H, W) as ctx:
        for host in (False, True):
            cut = list(streams)
            cut[35] = cut[35][:40]                                  # a truncated header, in the last batch
            rc, out = regrid_streams(ctx, cut, rows, cols, host=host)
            assert rc == 1 and "frame 35" in last_error() and out.untouched()
            rc, out = regrid_streams(ctx, [None] + list(streams[1:]), rows, cols, host=host)     # a frame without a stream
            assert rc == 1 and "frame 0" in last_error() and out.untouched()
            rc, out = regrid_streams(ctx, streams, M.AxisMap([H - 1], [2], [0.5, 0.5]), cols, host=host)      # a support that leaves the frame
            assert rc == 1 and last_error() and out.untouched()
        spec = M.regrid_spec(rows, cols)
        keep, ptrs, sizes = RG._args(streams)
        out = device_out(N, rows, cols)
        f = lib().ebcc_hip_regrid_shard
        assert f(ctx.ptr, ptrs, sizes, N, ctypes.byref(spec), out.ptr + 2) == 1 and last_error()      # out not 4-byte aligned
        assert f(ctx.ptr, ptrs, sizes, N, ctypes.byref(spec), None) == 1
        assert f(ctx.ptr, ptrs, sizes, 0, ctypes.byref(spec), out.ptr) == 1
        assert f(ctx.ptr, None, sizes, N, ctypes.byref(spec), out.ptr) == 1
        assert f(ctx.ptr, ptrs, None, N, ctypes.byref(spec), out.ptr) == 1
        assert f(ctx.ptr, ptrs, sizes, N, None, out.ptr) == 1
        assert f(None, ptrs, sizes, N, ctypes.byref(spec), out.ptr) == 1
        assert out.untouched()
    with L.Context(16, H, W) as ctx:
        for at in (1, 36):                                          # in the first batch of three; in the last
            bad = list(streams)
            bad[at] = damaged
            lo = at - at % 16
            keep, ptrs, sizes = RG._args(bad[lo:lo + 16])
            frames = L.DeviceArray(nbytes=16 * H * W * 4)
            refusal = lib().ebcc_hip_decode_frames(ctx.ptr, ptrs, sizes, len(keep), frames.ptr)       # the full decode of the batch
            frames.free()
            assert refusal != 0
            for host in (False, True):
                rc, out = regrid_streams(ctx, bad, rows, cols, host=host, base=1)
                assert rc == refusal and last_error() and out.sentinels_intact(), (at, host)
                rc, out = regrid_streams(ctx, streams, rows, cols, host=host, base=1)
                assert rc == 0, last_error()
                assert out.get().tobytes() == want and out.sentinels_intact(), f"after the damaged stream at {at}"


# ---- 4. Python -------------------------------------------------------------------------------------------------------------
def test_batch_codec_regrid(monkeypatch):
    HB.use_env(monkeypatch, {})
    from ebcc_amd import h5_batch
    streams, fields = catalogue()
    with h5_batch.BatchCodec(H, W, max_frames=16) as codec:
        for name, (rows, cols) in stream_maps().items():
            want = R.apply(fields, rows, cols)
            got = codec.regrid(streams, rows, cols)
            assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes(), name
            into = np.full(want.shape, JUNK, np.float32)
            assert codec.regrid(streams, rows, cols, out=into) is into and into.tobytes() == want.tobytes()
            dev = device_out(N, rows, cols, 1)                       # a device pointer: the shard form
            assert codec.regrid(streams, rows, cols, out=dev.ptr) == dev.ptr
            assert dev.get().tobytes() == want.tobytes() and dev.sentinels_intact()
        with pytest.raises(ValueError, match="outside the extent"):
            codec.regrid(streams, M.identity_map(H + 1), M.identity_map(W))
        with pytest.raises(ValueError):
            codec.regrid([], M.identity_map(H), M.identity_map(W))
        with pytest.raises(RuntimeError, match="frame 3"):
            codec.regrid(list(streams[:3]) + [streams[3][:40]], M.identity_map(H), M.identity_map(W))


def test_read_regridded_of_a_dataset(tmp_path):
    """h5_batch.read_regridded under an interpreter with h5py, as tests/test_series_gpu.py drives series_frames"""
    if not os.path.exists(T.CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([T.CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([T.CONDA_PY, os.path.join(L.ROOT, "tests", "h5_regrid.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 3, r.stdout
