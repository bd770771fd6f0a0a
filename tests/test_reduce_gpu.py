"""GPU: the reduce decode of include/ebcc_hip.h - ebcc_hip_time_fold (k_time_fold alone) and ebcc_hip_reduce_shard against a
plain Python loop over the frames in increasing index, in float64:

    acc = acc + x64;  acc2 = acc2 + x64 * x64;  np.minimum / np.maximum followed by + 0.0;  over += x > threshold in float32

on numpy's own arrays (kernel alone) or on the oracle's decode of the same streams.  Everything is compared by tobytes(): there
is no tolerance in this file.  The inputs make the order of the additions visible - the frames of a bin differ in scale by
factors of 1e6, so a float64 sum rounds - and every test that relies on that first asserts that its own expected fields, folded
in reverse order, give other bytes.

Not tested here: the refusal of a context for chunks of several frames - the C interface has no call that makes one (the audit's
tests leave it out for the same reason)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L
from tests import test_window_gpu as T

pytestmark = pytest.mark.gpu

NO_BIN = 0xFFFFFFFF
SENT = np.uint32(0xA5A5A5A5)
FRONT, BACK = 64, 37                                  # words of sentinel before (256 bytes) and behind
H, W = 64, 96
SCALES = (np.float32(1e-6), np.float32(1.0), np.float32(1e6))
FIELDS = (("d_sum", np.float64), ("d_sum_sq", np.float64), ("d_min", np.float32), ("d_max", np.float32), ("d_over", np.uint32))
THRESHOLD = 250.0


class TimeStats(ctypes.Structure):
    """ebcc_hip_time_stats"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("d_sum", ctypes.c_void_p), ("d_sum_sq", ctypes.c_void_p), ("d_min", ctypes.c_void_p), ("d_max", ctypes.c_void_p),
                ("d_over", ctypes.c_void_p), ("threshold", ctypes.c_float), ("count", ctypes.c_void_p)]


def lib():
    """the product with the reduce entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    p.ebcc_hip_time_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(TimeStats)]
    p.ebcc_hip_time_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(TimeStats)]
    p.ebcc_hip_reduce_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                        ctypes.POINTER(TimeStats)]
    p.ebcc_hip_window_plan.restype = ctypes.c_int
    p.ebcc_hip_window_plan.argtypes = [ctypes.c_size_t] * 6 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    for name in ("ebcc_hip_time_stats_init", "ebcc_hip_time_fold", "ebcc_hip_reduce_shard"):
        getattr(p, name).restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


class Guarded:
    """a host array on the device between sentinel words, beginning `base` 4-byte words behind a 256-byte boundary"""

    def __init__(self, host, base=0):
        host = np.ascontiguousarray(host)
        self.dtype, self.shape = host.dtype, host.shape
        body = host.view(np.uint32).ravel()
        self.at, self.n = FRONT + base, body.size
        self.words = np.concatenate([np.full(self.at, SENT, np.uint32), body, np.full(BACK, SENT, np.uint32)])
        self.d = L.DeviceArray(self.words)
        assert self.d.ptr % 256 == 0
        self.ptr = self.d.ptr + 4 * self.at

    def all(self):
        return self.d.get(np.uint32, self.words.shape)

    def get(self):
        return self.all()[self.at:self.at + self.n].view(self.dtype).reshape(self.shape)

    def sentinels_intact(self):
        a = self.all()
        return bool((a[:self.at] == SENT).all() and (a[self.at + self.n:] == SENT).all())

    def untouched(self):
        return np.array_equal(self.all(), self.words)


class Stats:
    """the accumulators [n_bins][rows][cols] on the device, every array between sentinels: the floats `base` words behind a
    256-byte boundary, the doubles 2 * base (8-byte aligned); `leave`: names left NULL.  Filled with junk until init()."""

    def __init__(self, n_bins, rows, cols, threshold=THRESHOLD, leave=(), base=0):
        self.shape = (n_bins, rows, cols)
        self.count = np.full(n_bins, 77, np.uint64)
        self.arrays = {name: Guarded(np.full(self.shape, 3, dtype), base * (2 if dtype == np.float64 else 1)) for name, dtype in FIELDS if name not in leave}
        self.c = TimeStats(n_bins, rows, cols, None, None, None, None, None, threshold, self.count.ctypes.data)
        for name, g in self.arrays.items():
            setattr(self.c, name, g.ptr)

    def init(self, ctx):
        assert lib().ebcc_hip_time_stats_init(ctx.ptr, ctypes.byref(self.c)) == 0, last_error()
        return self

    def get(self):
        """{name: bytes} of the accumulators and the count"""
        out = {name: g.get().tobytes() for name, g in self.arrays.items()}
        out["count"] = self.count.tobytes()
        return out

    def sentinels_intact(self):
        return all(g.sentinels_intact() for g in self.arrays.values())

    def snapshot(self):
        return [g.all().tobytes() for g in self.arrays.values()] + [self.count.tobytes()]


def expected(fields, bins, n_bins, threshold=THRESHOLD, order=None):
    """the loop the header states, on `fields` [n][rows][cols] float32 -> {name: bytes}; order: the frames' order (None: increasing)"""
    fields = np.asarray(fields, np.float32)
    shape = (n_bins,) + fields.shape[1:]
    s, s2 = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    mn, mx = np.full(shape, np.inf, np.float32), np.full(shape, -np.inf, np.float32)
    ov, count = np.zeros(shape, np.uint32), np.zeros(n_bins, np.uint64)
    for f in (range(len(fields)) if order is None else order):
        b = 0 if bins is None else int(bins[f])
        if b == NO_BIN:
            continue
        x = fields[f]
        x64 = x.astype(np.float64)
        s[b] = s[b] + x64
        s2[b] = s2[b] + x64 * x64
        mn[b] = np.minimum(mn[b], x) + np.float32(0.0)
        mx[b] = np.maximum(mx[b], x) + np.float32(0.0)
        ov[b] += x > np.float32(threshold)
        count[b] += 1
    return {"d_sum": s.tobytes(), "d_sum_sq": s2.tobytes(), "d_min": mn.tobytes(), "d_max": mx.tobytes(), "d_over": ov.tobytes(), "count": count.tobytes()}


def order_is_visible(fields, bins, n_bins):
    """folding the same fields in reverse order changes the bytes of both sums: a wrong order cannot pass"""
    fwd, rev = expected(fields, bins, n_bins), expected(fields, bins, n_bins, order=range(len(fields) - 1, -1, -1))
    return fwd["d_sum"] != rev["d_sum"] and fwd["d_sum_sq"] != rev["d_sum_sq"] and fwd["d_min"] == rev["d_min"] and fwd["count"] == rev["count"]


def same(got, want, what):
    for name in got:
        assert got[name] == want[name], (what, name)


# ---- 1. the kernel alone against numpy ---------------------------------------------------------------------------------------
KERNEL_BINS = [0, 1, 1, 0, 2]                          # a bin left and come back to, a repeat; bin 3 of 4 is never named


def kernel_items(h, w, n=5):
    """n items of N(5, 3) samples, scaled by 1e-6, 1, 1e6 in turn; -0 planted where it is a bin's minimum and maximum (KERNEL_BINS)"""
    r = np.random.default_rng(h * 1000 + w)
    x = np.stack([(r.standard_normal((h, w)) * 3 + 5).astype(np.float32) * SCALES[k % 3] for k in range(n)])
    x[1, 0, 0] = x[2, 0, 0] = -0.0                                  # bin 1: min and max are -0 -> +0 is written
    x[0, 0, 1], x[3, 0, 1] = 0.0, -0.0                              # bin 0: +0 then -0
    x[1:3, h - 1, w - 1] = np.abs(x[1:3, h - 1, w - 1])             # (the last pixel, a tail pixel where there is a tail)
    x[2, h - 1, w - 1] = -0.0                                      # bin 1: -0 is the minimum of (positive, -0)
    return x


def fold(ctx, items, bins, stats):
    b = None if bins is None else np.asarray(bins, np.uint32)
    return lib().ebcc_hip_time_fold(ctx.ptr, items.ptr, items.shape[0], None if b is None else b.ctypes.data, ctypes.byref(stats.c))


@pytest.mark.parametrize("h,w", [(37, 53), (64, 96), (90, 131)])          # (a tail of 1 pixel; none; a tail of 2 and more than one workgroup)
@pytest.mark.parametrize("base", [0, 1])
def test_kernel_against_numpy(h, w, base):
    x12 = kernel_items(h, w, 12)
    assert (h * w) % 4 == {37: 1, 64: 0, 90: 2}[h]
    # (the bins of the five items hold two frames at the most, and a + b is b + a: the order shows in a bin of twelve)
    assert order_is_visible(x12, None, 1)
    with L.Context(4, 64, 96) as ctx:                                # (any context of the device)
        runs = {}
        for what, bins in (("bins", KERNEL_BINS), ("skip", [0, 1, NO_BIN, 0, 2]), ("one bin", [0] * 12), ("no list", None)):
            n_bins = 4 if bins is not None and len(set(bins)) > 1 else 1
            x = x12[:5] if n_bins == 4 else x12
            items = Guarded(x, base)
            want = expected(x, bins, n_bins)
            st = Stats(n_bins, h, w, base=base).init(ctx)
            if n_bins == 4:                                           # (the initial values, which bin 3 keeps)
                start = expected(x[:0], [], 4)
                same(st.get(), start, "init")
            assert fold(ctx, items, bins, st) == 0, last_error()
            got = st.get()
            same(got, want, (what, h, w, base))
            if n_bins == 4:
                assert np.frombuffer(got["count"], np.uint64)[3] == 0
                for name, _ in FIELDS:
                    assert st.arrays[name].get()[3].tobytes() == np.frombuffer(start[name], st.arrays[name].dtype).reshape(st.shape)[3].tobytes()
            assert st.sentinels_intact() and items.untouched()
            runs[what] = got
            again = Stats(n_bins, h, w, base=base).init(ctx)          # a second run: the same bytes
            assert fold(ctx, items, bins, again) == 0
            assert again.get() == got
        assert runs["one bin"] == runs["no list"]
        assert np.frombuffer(runs["skip"]["count"], np.uint64).tolist() == [2, 1, 1, 0]
    # -0 counts as +0 and +0 is written
    mn = np.frombuffer(runs["bins"]["d_min"], np.float32).reshape(4, h, w)
    mx = np.frombuffer(runs["bins"]["d_max"], np.float32).reshape(4, h, w)
    zero = np.float32(0.0).tobytes()
    assert mn[1, 0, 0].tobytes() == zero and mx[1, 0, 0].tobytes() == zero and mn[1, h - 1, w - 1].tobytes() == zero


def test_kernel_results_do_not_depend_on_alignment():
    x = kernel_items(37, 53)
    with L.Context(4, 64, 96) as ctx:
        seen = set()
        for item_base in range(4):
            for base in (0, 1):
                st = Stats(4, 37, 53, base=base).init(ctx)
                assert fold(ctx, Guarded(x, item_base), KERNEL_BINS, st) == 0
                seen.add(tuple(sorted(st.get().items())))
        assert len(seen) == 1


@pytest.mark.parametrize("left", [name for name, _ in FIELDS])
def test_kernel_with_an_accumulator_left_null(left):
    h, w = 37, 53
    x = kernel_items(h, w)
    want = expected(x, KERNEL_BINS, 4)
    del want[left]
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 1)
        st = Stats(4, h, w, leave=(left,)).init(ctx)
        assert fold(ctx, items, KERNEL_BINS, st) == 0, last_error()
        got = st.get()
        assert left not in got
        same(got, want, left)
        assert st.sentinels_intact() and items.untouched()


def test_kernel_refusals_write_nothing():
    x = kernel_items(37, 53)
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 0)
        st = Stats(4, 37, 53).init(ctx)
        before = st.snapshot()
        assert fold(ctx, items, [0, 1, 4, 0, 2], st) == 1 and last_error()               # a bin >= n_bins
        assert fold(ctx, items, [NO_BIN] * 5, st) == 1 and last_error()                  # no item named
        assert lib().ebcc_hip_time_fold(ctx.ptr, items.ptr + 2, 5, None, ctypes.byref(st.c)) == 1     # items not 4-byte aligned
        assert lib().ebcc_hip_time_fold(ctx.ptr, None, 5, None, ctypes.byref(st.c)) == 1
        assert st.snapshot() == before and items.untouched()


# ---- 2. streams against the oracle, across batches ---------------------------------------------------------------------------
def scale_of(f):
    """1e-6, 1, 1e6 in turn, the turn shifted by one after every three frames: the frames f, f + 3, f + 6, .. of a bin
    f % 3 then differ in scale too"""
    return SCALES[(f + f // 3) % 3]


def _args(streams):
    """streams: bytes, or None for a frame that is not to be read (NULL, size 0)"""
    n = len(streams)
    bufs = [None if s is None else ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    ptrs = (ctypes.c_void_p * n)(*[None if b is None else ctypes.cast(b, ctypes.c_void_p).value for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in streams])
    return bufs, ptrs, sizes


def series(h, w, n):
    """n frames of h x w scaled as above, their streams from the product's encode (RELATIVE_ERROR: the bound follows each frame's
    range) and the oracle's decode of those streams; made once, never changed"""
    def make():
        L.oracle().orc_set_j2k_backend(0)
        x = np.stack([HB.inputs(h, w, [f])[0] * scale_of(f) for f in range(n)]).astype(np.float32)
        cfg = L.make_config((1, h, w), base_cr=20.0, error=0.004, residual_type=L.RELATIVE_ERROR)
        with L.Context(16, h, w) as ctx:
            streams = ctx.encode_frames(x, cfg)
        fields = np.stack([L.orc_decode(s).reshape(h, w) for s in streams])
        fields.setflags(write=False)
        return streams, fields
    return HB.once(("reduce series", h, w, n), make)


def reduce(ctx, streams, bins, stats, row0=0, col0=0):
    keep, ptrs, sizes = _args(streams)
    b = None if bins is None else np.asarray(bins, np.uint32)
    return lib().ebcc_hip_reduce_shard(ctx.ptr, ptrs, sizes, len(streams), None if b is None else b.ctypes.data, row0, col0, ctypes.byref(stats.c))


BINS12 = [f % 3 for f in range(12)]
ONE_BIN12 = [0] * 12                                  # (twelve frames in one bin: the order changes the sums at nearly half the pixels)


def one_bin(bins):
    return [NO_BIN if b == NO_BIN else 0 for b in bins]


def test_streams_against_the_oracle_across_batches(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)
    assert order_is_visible(fields, BINS12, 3) and order_is_visible(fields, ONE_BIN12, 1)
    for bins, n_bins in ((BINS12, 3), (ONE_BIN12, 1)):
        want = expected(fields, bins, n_bins)
        seen = []
        for cap in (5, 16, 5):                                      # three batches on two engine sets; one batch; the first again
            with L.Context(cap, H, W) as ctx:
                st = Stats(n_bins, H, W, base=1).init(ctx)
                assert reduce(ctx, streams, bins, st) == 0, last_error()
                got = st.get()
                same(got, want, f"capacity {cap}, {n_bins} bins")
                assert st.sentinels_intact()
                seen.append(got)
        assert seen[0] == seen[1] == seen[2]
        assert np.frombuffer(seen[0]["count"], np.uint64).tolist() == ([4, 4, 4] if n_bins == 3 else [12])


# ---- 3. a window ---------------------------------------------------------------------------------------------------------
def test_window(monkeypatch):
    HB.use_env(monkeypatch, {})
    h, w, (row0, col0, rows, cols) = 90, 131, (9, 50, 40, 30)       # (crosses the code-block boundary at column 64)
    streams, fields = series(h, w, 6)
    n = lib().ebcc_hip_window_plan(h, w, row0, col0, rows, cols, None, None, 0)
    blocks = np.zeros((n, 6), np.int32)
    assert n > 0 and lib().ebcc_hip_window_plan(h, w, row0, col0, rows, cols, None, blocks.ctypes.data, n) == n
    assert 0 < blocks[:, 5].sum() < n                               # a real window: fewer code-blocks than the frame has
    crop = fields[:, row0:row0 + rows, col0:col0 + cols]
    assert order_is_visible(crop, None, 1)
    want = expected(crop, None, 1)
    with L.Context(4, h, w) as ctx:                                 # (two batches)
        st = Stats(1, rows, cols).init(ctx)
        assert reduce(ctx, streams, None, st, row0, col0) == 0, last_error()
        same(st.get(), want, "window")
        assert st.sentinels_intact()
        # the window that is the frame runs the whole-frame decode
        whole = Stats(1, h, w).init(ctx)
        assert reduce(ctx, streams, None, whole) == 0, last_error()
        same(whole.get(), expected(fields, None, 1), "whole frame")


# ---- 4. skipped frames -----------------------------------------------------------------------------------------------------
def test_skipped_frames_are_not_read(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)
    bins, given = list(BINS12), list(streams)
    for f in (1, 4, 6, 11):
        bins[f], given[f] = NO_BIN, None
    assert order_is_visible(fields, one_bin(bins), 1)
    with L.Context(5, H, W) as ctx:                                 # (eight named frames: two batches)
        for layout, n_bins in ((bins, 3), (one_bin(bins), 1)):
            st = Stats(n_bins, H, W).init(ctx)
            assert reduce(ctx, given, layout, st) == 0, last_error()
            same(st.get(), expected(fields, layout, n_bins), f"skipped, {n_bins} bins")
            assert st.count.sum() == 8 and st.sentinels_intact()


# ---- 5. continuation -------------------------------------------------------------------------------------------------------
def test_a_series_split_over_two_calls(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)
    assert order_is_visible(fields, BINS12, 3) and order_is_visible(fields, ONE_BIN12, 1)
    with L.Context(5, H, W) as ctx:
        for bins, n_bins in ((BINS12, 3), (ONE_BIN12, 1)):
            st = Stats(n_bins, H, W).init(ctx)
            assert reduce(ctx, streams[:7], bins[:7], st) == 0, last_error()
            assert st.count.tolist() == [[7], None, [3, 2, 2]][n_bins - 1]
            assert reduce(ctx, streams[7:], bins[7:], st) == 0, last_error()
            same(st.get(), expected(fields, bins, n_bins), f"two calls, {n_bins} bins")


# ---- 6. special frames -----------------------------------------------------------------------------------------------------
def test_special_frames(monkeypatch):
    """a constant field, a frame without a residual layer and a legacy header-less stream in one list"""
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)

    def make():
        x = np.stack([np.full((H, W), 7.25e6, np.float32), HB.inputs(H, W, [20])[0]])
        with L.Context(4, H, W) as ctx:
            const = ctx.encode_frames(x[:1], L.make_config((1, H, W), base_cr=20.0, error=0.004, residual_type=L.RELATIVE_ERROR))[0]
            base_only = ctx.encode_frames(x[1:], L.make_config((1, H, W), base_cr=20.0, error=0.0, residual_type=L.NONE))[0]
        assert len(const) == 56
        return const, base_only
    const, base_only = HB.once("reduce special frames", make)
    mixed = [streams[0], const, L.legacy_repack(streams[1]), base_only, streams[2], streams[3]]
    decoded = np.stack([L.orc_decode(s).reshape(H, W) for s in mixed])
    assert np.array_equal(decoded[2], fields[1])
    want = expected(decoded, None, 1)
    with L.Context(4, H, W) as ctx:                                 # (two batches)
        st = Stats(1, H, W).init(ctx)
        assert reduce(ctx, mixed, None, st) == 0, last_error()
        same(st.get(), want, "special frames")


# ---- 7. refusals on the device ---------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)
    with L.Context(5, 90, 131) as other:                            # a context of another geometry
        st = Stats(3, H, W).init(other)
        before = st.snapshot()
        assert reduce(other, streams, BINS12, st) == 1 and last_error()
        assert st.snapshot() == before
    with L.Context(5, H, W) as ctx:
        st = Stats(3, H, W).init(ctx)
        before = st.snapshot()
        bad = list(streams)
        bad[10] = bad[10][:40]                                      # a truncated header, in the last batch
        assert reduce(ctx, bad, BINS12, st) == 1 and last_error()
        assert st.snapshot() == before
        assert reduce(ctx, streams, BINS12, st, row0=1) == 1 and last_error()             # the window leaves the frame
        assert reduce(ctx, streams, [0, 1, 3] * 4, st) == 1 and last_error()              # a bin >= n_bins
        assert reduce(ctx, [None] + list(streams[1:]), BINS12, st) == 1 and last_error()  # a named frame without a stream
        assert st.snapshot() == before
        # and the context still works
        assert reduce(ctx, streams, BINS12, st) == 0, last_error()
        same(st.get(), expected(fields, BINS12, 3), "after refusals")


def test_a_stream_damaged_inside_a_batch(monkeypatch):
    """The damaged stream of tests/test_codec_gpu.py::test_malformed_streams_are_rejected - its frame without a residual layer cut
    to 40 bytes, which reads as a legacy stream with eight bytes of codestream: the frame header parses, the decode of its batch
    refuses it.  The call returns 1, nothing outside the accumulators is written, and the next call on the context is correct."""
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)

    def make():
        with L.Context(4, H, W) as ctx:
            return ctx.encode_frames(L.era5_like(H, W, 64)[None], L.make_config((1, H, W), base_cr=10, residual_type=L.NONE))[0][:40]
    damaged = HB.once("reduce damaged stream", make)
    # in batch 1 of three, in the first - and in batch 1 of four: batch 2, on the other set, is waiting for the turn of the batch that
    # failed, and batch 3 only passes its turn on
    for cap, at in ((5, 8), (5, 1), (3, 4)):
        bad = list(streams)
        bad[at] = damaged
        with L.Context(cap, H, W) as ctx:
            st = Stats(3, H, W, base=1).init(ctx)
            assert reduce(ctx, bad, BINS12, st) == 1 and last_error()
            assert st.sentinels_intact()
            st.init(ctx)
            assert reduce(ctx, streams, BINS12, st) == 0, last_error()
            same(st.get(), expected(fields, BINS12, 3), f"after the damaged stream at {at} of batches of {cap}")
            assert st.sentinels_intact()


# ---- 8. h5py ---------------------------------------------------------------------------------------------------------------
def test_reduce_frames_of_a_dataset(tmp_path):
    """h5_batch.reduce_frames under an interpreter with h5py, as tests/test_box_decode_gpu.py drives read_boxes"""
    if not os.path.exists(T.CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([T.CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([T.CONDA_PY, os.path.join(L.ROOT, "tests", "h5_reduce.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 5, r.stdout
