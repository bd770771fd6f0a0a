"""GPU: the pair decode of include/ebcc_hip.h - ebcc_hip_pair_fold (k_pair_fold alone) and ebcc_hip_pair_shard against a plain
Python loop over the steps in increasing index, with a = x in float64 and b = y in float64:

    sum_x += a;  sum_y += b;  sum_xx += a * a;  sum_yy += b * b;  sum_xy += a * b
    m = sqrt(float32(a * a + b * b)) in float32;  sum_mag += float64(m);  max_mag = maximum(max_mag, m);  over_mag += m > threshold

on numpy's own arrays (kernel alone) or on the oracle's decode of the same streams.  Everything is compared by tobytes(): there
is no tolerance in this file.  The inputs make the order of the additions and the roundings of the magnitude visible - steps
differ in scale by factors of 1e6, and some steps pair fields of equal scale - and every test that relies on that first asserts
about its own expected arrays that the backward fold and two other magnitude formulas give other bytes.

Not tested here: the refusal of a context for chunks of several frames - the C interface has no call that makes one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L
from tests import test_reduce_gpu as R
from tests import test_window_gpu as T
from tests.test_reduce_gpu import Guarded, series, _args

pytestmark = pytest.mark.gpu

NO_BIN = R.NO_BIN
H, W = R.H, R.W
DOUBLES = ("d_sum_x", "d_sum_y", "d_sum_xx", "d_sum_yy", "d_sum_xy", "d_sum_mag")
FIELDS = tuple((name, np.float64) for name in DOUBLES) + (("d_max_mag", np.float32), ("d_over_mag", np.uint32))
MOMENTS = DOUBLES[:5]
MAGNITUDE = ("d_sum_mag", "d_max_mag", "d_over_mag")
THRESHOLD = 8.0                                        # (kernel items: magnitudes of about 7e-6, 7 and 7e6)
STREAM_THRESHOLD = 300.0                               # (the series: fields of about 250 times 1e-6, 1 or 1e6)


class PairStats(ctypes.Structure):
    """ebcc_hip_pair_stats"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("d_sum_x", ctypes.c_void_p), ("d_sum_y", ctypes.c_void_p), ("d_sum_xx", ctypes.c_void_p), ("d_sum_yy", ctypes.c_void_p),
                ("d_sum_xy", ctypes.c_void_p), ("d_sum_mag", ctypes.c_void_p), ("d_max_mag", ctypes.c_void_p), ("d_over_mag", ctypes.c_void_p),
                ("threshold", ctypes.c_float), ("count", ctypes.c_void_p)]


def lib():
    """the product with the pair entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = R.lib()
    p.ebcc_hip_pair_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(PairStats)]
    p.ebcc_hip_pair_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(PairStats)]
    p.ebcc_hip_pair_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                      ctypes.c_size_t, ctypes.POINTER(PairStats)]
    for name in ("ebcc_hip_pair_stats_init", "ebcc_hip_pair_fold", "ebcc_hip_pair_shard"):
        getattr(p, name).restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


last_error = R.last_error
same = R.same


class Stats:
    """the accumulators [n_bins][rows][cols] on the device, every array between sentinels: the 4-byte ones `base` words behind a
    256-byte boundary, the doubles 2 * base (8-byte aligned); `leave`: names left NULL.  Filled with junk until init()."""

    def __init__(self, n_bins, rows, cols, threshold=THRESHOLD, leave=(), base=0):
        self.shape = (n_bins, rows, cols)
        self.count = np.full(n_bins, 77, np.uint64)
        self.arrays = {name: Guarded(np.full(self.shape, 3, dtype), base * (2 if dtype == np.float64 else 1)) for name, dtype in FIELDS if name not in leave}
        self.c = PairStats(n_bins, rows, cols, None, None, None, None, None, None, None, None, threshold, self.count.ctypes.data)
        for name, g in self.arrays.items():
            setattr(self.c, name, g.ptr)

    def init(self, ctx):
        assert lib().ebcc_hip_pair_stats_init(ctx.ptr, ctypes.byref(self.c)) == 0, last_error()
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


def magnitude(a, b, formula="rule"):
    """m of the rule for a, b in float64 (widened float32) -> float32; the two formulas a kernel might use instead"""
    if formula == "rule":
        return np.sqrt((a * a + b * b).astype(np.float32))                    # (numpy's float32 square root is correctly rounded)
    if formula == "float":
        x, y = a.astype(np.float32), b.astype(np.float32)
        return np.sqrt(x * x + y * y)
    assert formula == "double"
    return np.sqrt(a * a + b * b).astype(np.float32)


def expected(xs, ys, bins, n_bins, threshold=THRESHOLD, order=None, formula="rule"):
    """the loop the header states, on xs and ys [n][rows][cols] float32 -> {name: bytes}; order: the steps' order (None: increasing)"""
    xs, ys = np.asarray(xs, np.float32), np.asarray(ys, np.float32)
    shape = (n_bins,) + xs.shape[1:]
    acc = {name: np.zeros(shape, np.float64) for name in DOUBLES}
    mx, ov, count = np.full(shape, -np.inf, np.float32), np.zeros(shape, np.uint32), np.zeros(n_bins, np.uint64)
    for t in (range(len(xs)) if order is None else order):
        k = 0 if bins is None else int(bins[t])
        if k == NO_BIN:
            continue
        a, b = xs[t].astype(np.float64), ys[t].astype(np.float64)
        m = magnitude(a, b, formula)
        assert m.dtype == np.float32
        for name, term in (("d_sum_x", a), ("d_sum_y", b), ("d_sum_xx", a * a), ("d_sum_yy", b * b), ("d_sum_xy", a * b), ("d_sum_mag", m.astype(np.float64))):
            acc[name][k] = acc[name][k] + term
        mx[k] = np.maximum(mx[k], m)
        ov[k] += m > np.float32(threshold)
        count[k] += 1
    out = {name: a.tobytes() for name, a in acc.items()}
    out.update({"d_max_mag": mx.tobytes(), "d_over_mag": ov.tobytes(), "count": count.tobytes()})
    return out


def the_rule_is_visible(xs, ys, bins, n_bins, threshold=THRESHOLD, mag_order=True):
    """about the expected arrays themselves: the backward fold gives other bytes for sum_xy and for sum_mag, and both other
    magnitude formulas give other bytes for sum_mag - a wrong order or a wrong rounding cannot pass.  (mag_order=False: bins
    of three steps at the most, whose magnitudes - 24-bit values 2^20 apart - mostly add up to the same double both ways;
    the order of sum_mag is then shown by the one-bin fold of the same items.)"""
    fwd = expected(xs, ys, bins, n_bins, threshold)
    rev = expected(xs, ys, bins, n_bins, threshold, order=range(len(xs) - 1, -1, -1))
    flt = expected(xs, ys, bins, n_bins, threshold, formula="float")
    dbl = expected(xs, ys, bins, n_bins, threshold, formula="double")
    return (fwd["d_sum_xy"] != rev["d_sum_xy"] and (fwd["d_sum_mag"] != rev["d_sum_mag"] or not mag_order) and fwd["count"] == rev["count"] and
            fwd["d_max_mag"] == rev["d_max_mag"] and fwd["d_sum_mag"] != flt["d_sum_mag"] and fwd["d_sum_mag"] != dbl["d_sum_mag"] and
            fwd["d_sum_xy"] == flt["d_sum_xy"])


# ---- 1. the kernel alone against numpy ---------------------------------------------------------------------------------------
KERNEL_BINS = [0, 1, NO_BIN, 0, 2, 1, 0]               # three bins, a bin left and come back to, a skipped item; bin 3 of 4 is never named
N_ITEMS = len(KERNEL_BINS)


def kernel_items(h, w, n=N_ITEMS):
    """n items of x and of y, N(5, 3) samples; x scaled by 1e-6, 1, 1e6 in turn, y the same for items 0..2 - equal scales: the
    roundings of the magnitude show - and a turn further for every three items after that"""
    def make():
        r = np.random.default_rng(h * 1000 + w)
        x = np.stack([(r.standard_normal((h, w)) * 3 + 5).astype(np.float32) * R.SCALES[k % 3] for k in range(n)])
        y = np.stack([(r.standard_normal((h, w)) * 3 + 5).astype(np.float32) * R.SCALES[(k + k // 3) % 3] for k in range(n)])
        x.setflags(write=False)
        y.setflags(write=False)
        return x, y
    return HB.once(("pair kernel items", h, w, n), make)


def kernel_want(h, w, bins, n_bins):
    x, y = kernel_items(h, w)
    return HB.once(("pair kernel want", h, w, tuple(bins) if bins is not None else None, n_bins), lambda: expected(x, y, bins, n_bins))


def fold(ctx, x_items, y_items, bins, stats, n=None):
    b = None if bins is None else np.asarray(bins, np.uint32)
    return lib().ebcc_hip_pair_fold(ctx.ptr, x_items.ptr, y_items.ptr, x_items.shape[0] if n is None else n, None if b is None else b.ctypes.data,
                                    ctypes.byref(stats.c))


@pytest.mark.parametrize("h,w", [(37, 53), (64, 96), (90, 131)])          # (a tail of 1 pixel; none; a tail of 2 and more than one workgroup)
@pytest.mark.parametrize("base", [0, 1])
def test_kernel_against_numpy(h, w, base):
    x, y = kernel_items(h, w)
    assert (h * w) % 4 == {37: 1, 64: 0, 90: 2}[h]
    assert the_rule_is_visible(x, y, None, 1) and the_rule_is_visible(x, y, KERNEL_BINS, 4, mag_order=False)
    with L.Context(4, 64, 96) as ctx:                                # (any context of the device)
        start = expected(x[:0], y[:0], [], 4)
        for what, bins, n_bins in (("bins", KERNEL_BINS, 4), ("no list", None, 1)):
            xi, yi = Guarded(x, base), Guarded(y, base)
            want = kernel_want(h, w, bins, n_bins)
            st = Stats(n_bins, h, w, base=base).init(ctx)
            if n_bins == 4:                                           # (the initial values, which bin 3 keeps)
                same(st.get(), start, "init")
            assert fold(ctx, xi, yi, bins, st) == 0, last_error()
            got = st.get()
            same(got, want, (what, h, w, base))
            if n_bins == 4:
                assert np.frombuffer(got["count"], np.uint64).tolist() == [3, 2, 1, 0]
                for name, _ in FIELDS:
                    assert st.arrays[name].get()[3].tobytes() == np.frombuffer(start[name], st.arrays[name].dtype).reshape(st.shape)[3].tobytes()
                assert 0 < np.frombuffer(got["d_over_mag"], np.uint32).sum() < 6 * h * w
            assert st.sentinels_intact() and xi.untouched() and yi.untouched()
            again = Stats(n_bins, h, w, base=base).init(ctx)          # a second run: the same bytes
            assert fold(ctx, xi, yi, bins, again) == 0
            assert again.get() == got


# ---- 2. alignment ------------------------------------------------------------------------------------------------------------
def test_kernel_results_do_not_depend_on_alignment():
    h, w = 37, 53
    x, y = kernel_items(h, w)
    want = kernel_want(h, w, KERNEL_BINS, 4)
    with L.Context(4, 64, 96) as ctx:
        for x_base, y_base in ((0, 0), (1, 0), (0, 3), (2, 1)):       # (each side on a 16-byte boundary and off it)
            xi, yi = Guarded(x, x_base), Guarded(y, y_base)
            assert (xi.ptr % 16 == 0) == (x_base == 0) and (yi.ptr % 16 == 0) == (y_base == 0)
            st = Stats(4, h, w, base=x_base % 2).init(ctx)
            assert fold(ctx, xi, yi, KERNEL_BINS, st) == 0, last_error()
            same(st.get(), want, (x_base, y_base))
            assert st.sentinels_intact() and xi.untouched() and yi.untouched()


# ---- 3. accumulators left NULL -----------------------------------------------------------------------------------------------
SUBSETS = [("moments only", MOMENTS), ("magnitude only", MAGNITUDE)] + [(name, (name,)) for name, _ in FIELDS]


@pytest.mark.parametrize("what,kept", SUBSETS, ids=[s[0] for s in SUBSETS])
def test_kernel_with_accumulators_left_null(what, kept):
    h, w = 37, 53
    x, y = kernel_items(h, w)
    full = kernel_want(h, w, KERNEL_BINS, 4)
    want = {name: full[name] for name in tuple(kept) + ("count",)}
    with L.Context(4, 64, 96) as ctx:
        xi, yi = Guarded(x, 1), Guarded(y, 0)
        st = Stats(4, h, w, leave=[name for name, _ in FIELDS if name not in kept]).init(ctx)
        assert fold(ctx, xi, yi, KERNEL_BINS, st) == 0, last_error()
        got = st.get()
        assert sorted(got) == sorted(want)
        same(got, want, what)
        assert st.sentinels_intact() and xi.untouched() and yi.untouched()


# ---- 4. x and y the same array -------------------------------------------------------------------------------------------------
def test_kernel_with_the_same_items_twice():
    h, w = 37, 53
    x, _ = kernel_items(h, w)
    with L.Context(4, 64, 96) as ctx:
        xi = Guarded(x, 1)
        st = Stats(4, h, w).init(ctx)
        assert fold(ctx, xi, xi, KERNEL_BINS, st) == 0, last_error()
        got = st.get()
        same(got, expected(x, x, KERNEL_BINS, 4), "x twice")
        alone = R.Stats(4, h, w).init(ctx)
        assert R.fold(ctx, xi, KERNEL_BINS, alone) == 0, last_error()
        one = alone.get()
        assert got["d_sum_xy"] == got["d_sum_xx"] == got["d_sum_yy"] == one["d_sum_sq"]
        assert got["d_sum_x"] == got["d_sum_y"] == one["d_sum"] and got["count"] == one["count"]
        assert xi.untouched()


# ---- 5. a list longer than one launch ------------------------------------------------------------------------------------------
def test_a_list_longer_than_one_launch():
    n = 65536 + 3
    r = np.random.default_rng(5)
    scale = np.asarray(R.SCALES, np.float32)
    x = (r.standard_normal((n, 1, 5)) * 3 + 5).astype(np.float32) * scale[np.arange(n) % 3][:, None, None]
    y = (r.standard_normal((n, 1, 5)) * 3 + 5).astype(np.float32) * scale[(np.arange(n) // 2) % 3][:, None, None]
    bins = (np.arange(n) % 5 == 0).astype(np.uint32)                  # (bin 1: 13108 entries, bin 0: 52431 - its run is cut by the launch)
    want = expected(x, y, bins, 2)
    assert want["d_sum_xy"] != expected(x, y, bins, 2, order=range(n - 1, -1, -1))["d_sum_xy"]
    with L.Context(4, 64, 96) as ctx:
        xi, yi = Guarded(x, 1), Guarded(y, 2)
        st = Stats(2, 1, 5, base=1).init(ctx)
        assert fold(ctx, xi, yi, bins, st) == 0, last_error()
        same(st.get(), want, "65539 items")
        assert st.sentinels_intact() and xi.untouched() and yi.untouched()


# ---- 6. refusals of the kernel call ----------------------------------------------------------------------------------------------
def test_kernel_refusals_write_nothing():
    x, y = kernel_items(37, 53)
    with L.Context(4, 64, 96) as ctx:
        xi, yi = Guarded(x, 0), Guarded(y, 0)
        st = Stats(4, 37, 53).init(ctx)
        before = st.snapshot()
        f = lib().ebcc_hip_pair_fold
        assert fold(ctx, xi, yi, [0, 1, 4, 0, 2, 1, 0], st) == 1 and "ebcc_hip_pair_fold" in last_error()    # a bin >= n_bins
        assert fold(ctx, xi, yi, [NO_BIN] * N_ITEMS, st) == 1 and last_error()                               # no item named
        assert f(ctx.ptr, xi.ptr + 2, yi.ptr, N_ITEMS, None, ctypes.byref(st.c)) == 1 and last_error()       # x not 4-byte aligned
        assert f(ctx.ptr, xi.ptr, yi.ptr + 1, N_ITEMS, None, ctypes.byref(st.c)) == 1 and last_error()       # y not 4-byte aligned
        assert f(ctx.ptr, None, yi.ptr, N_ITEMS, None, ctypes.byref(st.c)) == 1 and last_error()
        assert f(ctx.ptr, xi.ptr, None, N_ITEMS, None, ctypes.byref(st.c)) == 1 and last_error()
        assert f(ctx.ptr, xi.ptr, yi.ptr, N_ITEMS, None, None) == 1 and last_error()
        st.c.threshold = float("nan")
        assert fold(ctx, xi, yi, KERNEL_BINS, st) == 1 and "threshold" in last_error()                       # a NaN threshold with d_over_mag
        st.c.threshold = THRESHOLD
        st.c.d_sum_mag += 4
        assert fold(ctx, xi, yi, KERNEL_BINS, st) == 1 and "8-byte" in last_error()                          # a misaligned double array
        st.c.d_sum_mag -= 4
        assert st.snapshot() == before and xi.untouched() and yi.untouched()
        assert fold(ctx, xi, yi, KERNEL_BINS, st) == 0, last_error()                                         # and the call still works
        same(st.get(), kernel_want(37, 53, KERNEL_BINS, 4), "after refusals")


# ---- 7. streams against the oracle, across batches ---------------------------------------------------------------------------
N_STEPS = 8
BINS8 = [t % 3 for t in range(N_STEPS)]
ONE_BIN8 = [0] * N_STEPS


def pairs():
    """(x streams, y streams, x fields, y fields): frames 0..7 and 4..11 of the reduce decode's series - steps 2 and 5 pair
    frames of equal scale, the others differ by 1e6"""
    streams, fields = series(H, W, 12)
    assert [R.scale_of(t) == R.scale_of(t + 4) for t in range(N_STEPS)] == [t in (2, 5) for t in range(N_STEPS)]
    return list(streams[:8]), list(streams[4:12]), fields[:8], fields[4:12]


def stream_want(bins, n_bins):
    sx, sy, fx, fy = pairs()
    return HB.once(("pair stream want", tuple(bins), n_bins), lambda: expected(fx, fy, bins, n_bins, STREAM_THRESHOLD))


def pair(ctx, xs, ys, bins, stats, row0=0, col0=0):
    keep_x, px, zx = _args(xs)
    keep_y, py, zy = (keep_x, px, zx) if ys is xs else _args(ys)
    b = None if bins is None else np.asarray(bins, np.uint32)
    return lib().ebcc_hip_pair_shard(ctx.ptr, px, zx, py, zy, len(xs), None if b is None else b.ctypes.data, row0, col0, ctypes.byref(stats.c))


def test_streams_against_the_oracle_across_batches(monkeypatch):
    HB.use_env(monkeypatch, {})
    sx, sy, fx, fy = pairs()
    assert the_rule_is_visible(fx, fy, ONE_BIN8, 1, STREAM_THRESHOLD)
    for bins, n_bins in ((BINS8, 3), (ONE_BIN8, 1)):
        want = stream_want(bins, n_bins)
        assert 0 < np.frombuffer(want["d_over_mag"], np.uint32).sum() < N_STEPS * H * W
        seen = []
        for cap in (3, 6, 16, 3):                                   # a step a batch on two engine sets (an odd capacity); three batches; one; the first again
            with L.Context(cap, H, W) as ctx:
                st = Stats(n_bins, H, W, STREAM_THRESHOLD, base=1).init(ctx)
                assert pair(ctx, sx, sy, bins, st) == 0, last_error()
                got = st.get()
                same(got, want, f"capacity {cap}, {n_bins} bins")
                assert st.sentinels_intact()
                seen.append(got)
        assert seen[0] == seen[1] == seen[2] == seen[3]
        assert np.frombuffer(seen[0]["count"], np.uint64).tolist() == ([3, 3, 2] if n_bins == 3 else [8])


# ---- 8. the shard call equals the kernel on the decoded fields ------------------------------------------------------------------
def test_the_shard_call_equals_the_kernel_on_the_decoded_fields(monkeypatch):
    HB.use_env(monkeypatch, {})
    sx, sy, fx, fy = pairs()
    with L.Context(6, H, W) as ctx:
        a = Stats(3, H, W, STREAM_THRESHOLD).init(ctx)
        assert pair(ctx, sx, sy, BINS8, a) == 0, last_error()
        b = Stats(3, H, W, STREAM_THRESHOLD, base=1).init(ctx)
        assert fold(ctx, Guarded(fx, 1), Guarded(fy, 0), BINS8, b) == 0, last_error()
        assert a.get() == b.get()
        # x_streams == y_streams: sum_xy carries the bytes of sum_xx
        c = Stats(3, H, W, STREAM_THRESHOLD).init(ctx)
        assert pair(ctx, sx, sx, BINS8, c) == 0, last_error()
        got = c.get()
        assert got["d_sum_xy"] == got["d_sum_xx"] == got["d_sum_yy"] == a.get()["d_sum_xx"] and got["d_sum_x"] == got["d_sum_y"]


# ---- 9. a window -----------------------------------------------------------------------------------------------------------
def test_window(monkeypatch):
    HB.use_env(monkeypatch, {})
    row0, col0, rows, cols = 9, 50, 40, 30                          # (rows 9..49, columns 50..80: crosses the code-block boundary at column 64)
    sx, sy, fx, fy = pairs()
    whole = stream_want(BINS8, 3)
    want = {}
    for name, dtype in FIELDS:
        want[name] = np.frombuffer(whole[name], dtype).reshape(3, H, W)[:, row0:row0 + rows, col0:col0 + cols].tobytes()
    want["count"] = whole["count"]
    assert want == expected(fx[:, row0:row0 + rows, col0:col0 + cols], fy[:, row0:row0 + rows, col0:col0 + cols], BINS8, 3, STREAM_THRESHOLD)
    with L.Context(6, H, W) as ctx:
        st = Stats(3, rows, cols, STREAM_THRESHOLD, base=1).init(ctx)
        assert pair(ctx, sx, sy, BINS8, st, row0, col0) == 0, last_error()
        same(st.get(), want, "window")
        assert st.sentinels_intact()


# ---- 10. skipped steps -------------------------------------------------------------------------------------------------------
def test_skipped_steps_are_not_read(monkeypatch):
    HB.use_env(monkeypatch, {})
    sx, sy, fx, fy = pairs()
    bins = list(BINS8)
    for t in (1, 4, 7):
        bins[t], sx[t], sy[t] = NO_BIN, None, None
    with L.Context(4, H, W) as ctx:                                 # (five named steps: three batches)
        st = Stats(3, H, W, STREAM_THRESHOLD).init(ctx)
        assert pair(ctx, sx, sy, bins, st) == 0, last_error()
        same(st.get(), expected(fx, fy, bins, 3, STREAM_THRESHOLD), "skipped")
        assert st.count.tolist() == [3, 0, 2] and st.sentinels_intact()


# ---- 11. continuation --------------------------------------------------------------------------------------------------------
def test_a_series_split_over_two_calls(monkeypatch):
    HB.use_env(monkeypatch, {})
    sx, sy, fx, fy = pairs()
    with L.Context(4, H, W) as ctx:
        for bins, n_bins in ((BINS8, 3), (ONE_BIN8, 1)):
            st = Stats(n_bins, H, W, STREAM_THRESHOLD).init(ctx)
            assert pair(ctx, sx[:5], sy[:5], bins[:5], st) == 0, last_error()
            assert st.count.tolist() == ([2, 2, 1] if n_bins == 3 else [5])
            assert pair(ctx, sx[5:], sy[5:], bins[5:], st) == 0, last_error()
            same(st.get(), stream_want(bins, n_bins), f"two calls, {n_bins} bins")


# ---- 12. refusals on the device ------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(monkeypatch):
    HB.use_env(monkeypatch, {})
    sx, sy, fx, fy = pairs()
    with L.Context(1, H, W) as one:                                 # a context of capacity 1
        st = Stats(3, H, W, STREAM_THRESHOLD).init(one)
        before = st.snapshot()
        assert pair(one, sx, sy, BINS8, st) == 1 and "capacity 1" in last_error()
        assert st.snapshot() == before
    with L.Context(6, H, W) as ctx:
        st = Stats(3, H, W, STREAM_THRESHOLD).init(ctx)
        before = st.snapshot()
        assert pair(ctx, sx, sy[:6] + [None] + sy[7:], BINS8, st) == 1                    # a named step without its y stream
        assert "step 6" in last_error() and " y " in last_error()
        bad = list(sx)
        bad[7] = bad[7][:40]                                        # a truncated header in x, in the last batch
        assert pair(ctx, bad, sy, BINS8, st) == 1
        assert "step 7" in last_error() and " x " in last_error()
        st.c.d_sum_xy += 4                                          # a misaligned d_sum_xy
        assert pair(ctx, sx, sy, BINS8, st) == 1 and "8-byte" in last_error()
        st.c.d_sum_xy -= 4
        assert pair(ctx, sx, sy, BINS8, st, row0=1) == 1 and last_error()                 # the window leaves the frame
        assert pair(ctx, sx, sy, [0, 1, 3] * 2 + [0, 1], st) == 1 and last_error()        # a bin >= n_bins
        assert st.snapshot() == before
        # and the context still works
        assert pair(ctx, sx, sy, BINS8, st) == 0, last_error()
        same(st.get(), stream_want(BINS8, 3), "after refusals")


# ---- 13. a stream damaged inside a batch ---------------------------------------------------------------------------------------
def test_a_stream_damaged_inside_a_later_batch(monkeypatch):
    """The damaged stream of tests/test_reduce_gpu.py: the frame header parses, the decode of its batch refuses it.  The call
    returns 1, count is what it was, nothing outside the accumulators is written, and the next call on the context is correct."""
    HB.use_env(monkeypatch, {})
    sx, sy, fx, fy = pairs()

    def make():
        with L.Context(4, H, W) as ctx:
            return ctx.encode_frames(L.era5_like(H, W, 64)[None], L.make_config((1, H, W), base_cr=10, residual_type=L.NONE))[0][:40]
    damaged = HB.once("reduce damaged stream", make)
    for cap, t, side in ((6, 5, "y"), (3, 4, "x")):                 # in batch 1 of three; in batch 4 of eight, one step a batch
        bx, by = list(sx), list(sy)
        (bx if side == "x" else by)[t] = damaged
        with L.Context(cap, H, W) as ctx:
            st = Stats(3, H, W, STREAM_THRESHOLD, base=1).init(ctx)
            assert pair(ctx, sx[:2], sy[:2], BINS8[:2], st) == 0, last_error()
            assert st.count.tolist() == [1, 1, 0]
            assert pair(ctx, bx, by, BINS8, st) == 1 and last_error()
            assert st.count.tolist() == [1, 1, 0] and st.sentinels_intact()
            st.init(ctx)
            assert pair(ctx, sx, sy, BINS8, st) == 0, last_error()
            same(st.get(), stream_want(BINS8, 3), f"after the damaged {side} stream at step {t}, batches of {cap}")
            assert st.sentinels_intact()


# ---- 14. the reduce decode's bytes ---------------------------------------------------------------------------------------------
def test_sum_x_and_sum_xx_are_the_reduce_decode_of_x(monkeypatch):
    HB.use_env(monkeypatch, {})
    sx, sy, fx, fy = pairs()
    with L.Context(5, H, W) as ctx:
        st = Stats(3, H, W, STREAM_THRESHOLD, leave=MAGNITUDE).init(ctx)
        assert pair(ctx, sx, sy, BINS8, st) == 0, last_error()
        for streams, s, s2 in ((sx, "d_sum_x", "d_sum_xx"), (sy, "d_sum_y", "d_sum_yy")):
            alone = R.Stats(3, H, W).init(ctx)
            assert R.reduce(ctx, streams, BINS8, alone) == 0, last_error()
            assert st.get()[s] == alone.get()["d_sum"] and st.get()[s2] == alone.get()["d_sum_sq"] and st.get()["count"] == alone.get()["count"]


# ---- 15. Python ------------------------------------------------------------------------------------------------------------------
def test_batch_codec_pair_with_a_state(monkeypatch):
    HB.use_env(monkeypatch, {})
    from ebcc_amd import h5_batch as B
    sx, sy, fx, fy = pairs()
    want = stream_want(BINS8, 3)
    names = {"sum_x": "d_sum_x", "sum_y": "d_sum_y", "sum_xx": "d_sum_xx", "sum_yy": "d_sum_yy", "sum_xy": "d_sum_xy", "sum_mag": "d_sum_mag",
             "max_mag": "d_max_mag", "over_mag": "d_over_mag", "count": "count"}
    with B.BatchCodec(H, W, max_frames=5) as codec:
        with codec.pair_state(3, threshold=STREAM_THRESHOLD) as state:
            assert codec.pair(sx[:3], sy[:3], bins=BINS8[:3], state=state) is state
            codec.pair(sx[3:], sy[3:], bins=BINS8[3:], state=state)
            got = state.result()
        for attr, name in names.items():
            assert getattr(got, attr).tobytes() == want[name], attr
        one = codec.pair(sx, sy, bins=BINS8, n_bins=3, threshold=STREAM_THRESHOLD)
        for attr, name in names.items():
            assert getattr(one, attr).tobytes() == want[name], attr
        n = got.count.astype(np.float64)[:, None, None]
        assert got.mean_x.dtype == np.float64 and got.mean_x.tobytes() == (got.sum_x / n).tobytes() and got.mean_mag.tobytes() == (got.sum_mag / n).tobytes()
        assert got.cov.tobytes() == (got.sum_xy / n - got.mean_x * got.mean_y).tobytes()
        r = got.corr
        assert np.isfinite(r).any() and (np.abs(r[np.isfinite(r)]) <= 1 + 1e-9).all()
        # co-moments only: no magnitude array; a bin without steps: NaN
        bins = [0 if b == 0 else -1 for b in BINS8]
        bare = codec.pair(sx, [None if b < 0 else s for b, s in zip(bins, sy)], bins=bins, n_bins=2, magnitude=False)
        assert bare.sum_mag is None and bare.max_mag is None and bare.over_mag is None and bare.mean_mag is None
        assert bare.count.tolist() == [3, 0] and bare.sum_xy[0].tobytes() == got.sum_xy[0].tobytes()
        assert np.isnan(bare.mean_x[1]).all() and np.isnan(bare.cov[1]).all() and np.isnan(bare.corr[1]).all()
        same_twice = codec.pair(sx, sx, magnitude=False)
        assert same_twice.sum_xy.tobytes() == same_twice.sum_xx.tobytes()
        for bad in (dict(bins=[0] * 7), dict(bins=[-1] * 8), dict(bins=[3] * 8, n_bins=3), dict(threshold=float("nan")), dict(threshold=1.0, magnitude=False)):
            with pytest.raises(ValueError):
                codec.pair(sx, sy, **bad)
        with pytest.raises(ValueError):
            codec.pair(sx, sy[:7])
    with B.BatchCodec(H, W, max_frames=1) as codec, pytest.raises(RuntimeError, match="capacity 1"):
        codec.pair(sx, sy)


def test_pair_frames_of_two_datasets(tmp_path):
    """h5_batch.pair_frames under an interpreter with h5py, as tests/test_reduce_gpu.py drives reduce_frames"""
    from ebcc_amd import h5_batch
    assert callable(h5_batch.pair_frames)                           # (missing: a failure, not a skip)
    if not os.path.exists(T.CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([T.CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([T.CONDA_PY, os.path.join(L.ROOT, "tests", "h5_pair.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 4, r.stdout
