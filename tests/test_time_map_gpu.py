"""GPU: the time-map decode of include/ebcc_hip.h - ebcc_hip_time_map_items (k_time_map alone) and ebcc_hip_project_shard against
a plain Python loop over every output's terms in the order of the map, in float64:

    acc = acc + w * x.astype(float64)          (the product rounds, then the sum rounds: never an FMA)

on numpy's own arrays (kernel alone) or on the oracle's decode of the same streams.  Everything is compared by tobytes(): there
is no tolerance in this file, and no NaN among the inputs.  The inputs make the rule visible - the frames differ in scale by
factors of 1e6 and the weights are such as 1/3, -2/7 and 0.1 - and every test that relies on the order first asserts about its
own expected arrays that the terms folded backwards give other bytes, and that the unrounded product (exact rationals on a
handful of pixels, rounded once: what an FMA computes) gives other bytes too.

Sentinel buffers and the stream fixtures are those of tests/test_reduce_gpu.py.  Not tested here: the refusal of a context for
chunks of several frames - the C interface has no call that makes one (the reduce decode's tests leave it out for the same
reason)."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L
from tests import test_reduce_gpu as R
from tests import test_window_gpu as T

pytestmark = pytest.mark.gpu

H, W = 64, 96
WEIGHTS = (1.0 / 3.0, -2.0 / 7.0, 0.1)
JUNK = 3.0                                            # what the accumulators hold before init


class TimeMap(ctypes.Structure):
    """ebcc_hip_time_map"""
    _fields_ = [("n_out", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t), ("start", ctypes.c_void_p),
                ("frame", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("d_acc", ctypes.c_void_p), ("count", ctypes.c_void_p)]


def lib():
    """the product with the time-map entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    p.ebcc_hip_time_map_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(TimeMap)]
    p.ebcc_hip_time_map_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(TimeMap)]
    p.ebcc_hip_project_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                         ctypes.POINTER(TimeMap)]
    for name in ("ebcc_hip_time_map_init", "ebcc_hip_time_map_items", "ebcc_hip_project_shard"):
        getattr(p, name).restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


last_error = R.last_error


# ---- maps: (start, frame, weight) ------------------------------------------------------------------------------------------------
def weight_of(o, k):
    return WEIGHTS[(o + k) % 3] * (1 + o)


def terms_of(rows):
    """rows: for every output the list of its (frame, weight) terms"""
    start = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    frame = np.array([f for r in rows for f, _ in r], np.uint32)
    weight = np.array([w for r in rows for _, w in r], np.float64)
    return start, frame, weight


def dense_map(n_out, n_items, leave=()):
    """every output names every item; leave: (output, item) terms taken out"""
    return terms_of([[(k, weight_of(o, k)) for k in range(n_items) if (o, k) not in leave] for o in range(n_out)])


def banded_map(n_items, width):
    return terms_of([[(k, weight_of(o, k)) for k in range(o, o + width)] for o in range(n_items - width + 1)])


def rebased(terms, lo, hi):
    """the terms with a frame in [lo, hi), counted from lo"""
    start, frame, weight = terms
    rows = [[(int(frame[t]) - lo, weight[t]) for t in range(int(start[o]), int(start[o + 1])) if lo <= frame[t] < hi] for o in range(len(start) - 1)]
    return terms_of(rows)


class Map:
    """a map's terms on the host and its accumulators [n_out][rows][cols] on the device between sentinels, 2 * base words behind a
    256-byte boundary (8-byte aligned); filled with JUNK until init(), count with 77"""

    def __init__(self, terms, rows, cols, base=0):
        self.start, self.frame, self.weight = terms
        self.n_out = len(self.start) - 1
        self.count = np.full(self.n_out, 77, np.uint64)
        self.acc = R.Guarded(np.full((self.n_out, rows, cols), JUNK, np.float64), 2 * base)
        assert self.acc.ptr % 8 == 0
        self.c = TimeMap(self.n_out, rows, cols, self.start.ctypes.data, self.frame.ctypes.data, self.weight.ctypes.data, self.acc.ptr,
                         self.count.ctypes.data)

    def with_terms(self, terms):
        """the same accumulators under other terms (a later call of a series)"""
        other = object.__new__(Map)
        other.__dict__.update(self.__dict__)
        other.start, other.frame, other.weight = terms
        assert len(other.start) - 1 == self.n_out
        other.c = TimeMap(self.n_out, self.c.rows, self.c.cols, other.start.ctypes.data, other.frame.ctypes.data, other.weight.ctypes.data,
                          self.acc.ptr, self.count.ctypes.data)
        return other

    def init(self, ctx):
        assert lib().ebcc_hip_time_map_init(ctx.ptr, ctypes.byref(self.c)) == 0, last_error()
        return self

    def get(self):
        return self.acc.get().tobytes()

    def snapshot(self):
        return [self.acc.all().tobytes(), self.count.tobytes()]


def expected(fields, terms, init=0.0, order=1):
    """the loop the header states, on `fields` [n][rows][cols] float32 -> float64 [n_out][rows][cols]; order -1: every output's
    terms backwards"""
    start, frame, weight = terms
    acc = np.full((len(start) - 1,) + fields.shape[1:], init, np.float64)
    x64 = np.asarray(fields, np.float32).astype(np.float64)         # (exact, made once)
    for o in range(len(start) - 1):
        for t in range(int(start[o]), int(start[o + 1]))[::order]:
            acc[o] = acc[o] + weight[t] * x64[frame[t]]
    return acc


def counts(terms):
    return np.diff(terms[0].astype(np.int64)).astype(np.uint64)


def rule_is_visible(fields, terms, pixels=12):
    """about the expected arrays themselves: the terms folded backwards give other bytes, and so does the product left unrounded -
    acc = round(acc + w * x) in exact rationals, which is what an FMA computes - on the first `pixels` pixels of the widest output"""
    start, frame, weight = terms
    fwd = expected(fields, terms)
    if fwd.tobytes() == expected(fields, terms, order=-1).tobytes():
        return False
    o = int(np.argmax(np.diff(start.astype(np.int64))))
    flat = fields.reshape(len(fields), -1)
    fused = []
    for p in range(pixels):
        acc = 0.0
        for t in range(int(start[o]), int(start[o + 1])):
            acc = float(Fraction(acc) + Fraction(float(weight[t])) * Fraction(float(flat[frame[t], p])))
        fused.append(acc)
    return np.array(fused).tobytes() != fwd[o].reshape(-1)[:pixels].tobytes()


# ---- 1. the kernel alone against numpy ---------------------------------------------------------------------------------------
def kernel_items(h, w, n=12):
    """n items of N(5, 3) samples, scaled by 1e-6, 1, 1e6 in turn"""
    r = np.random.default_rng(h * 1000 + w)
    return np.stack([(r.standard_normal((h, w)) * 3 + 5).astype(np.float32) * R.SCALES[k % 3] for k in range(n)])


def kernel_maps():
    """{name: (terms, items used, how the list runs)}"""
    return {
        "dense 5": (dense_map(5, 12), 12, "groups of 4 + 1"),
        "dense 5, one term less": (dense_map(5, 12, leave={(2, 7)}), 12, "outputs 0-1 and 3-4 as groups, output 2 alone"),
        "banded": (banded_map(9, 3), 9, "seven groups of one"),
        "an output without terms, an unnamed item": (terms_of([[(k, weight_of(0, k)) for k in range(12) if k != 4], [],
                                                               [(k, weight_of(2, k)) for k in range(12) if k != 4]]), 12, "groups of one around a gap"),
        "mixed": (terms_of([[(k, weight_of(o, k)) for k in range(12)] for o in range(3)] + [[(3, 0.1), (5, -0.7)]] +
                           [[(k, weight_of(o, k)) for k in range(2, 9)] for o in range(6)]), 12, "3, 1, 4, 2"),
        "one item": (terms_of([[(0, 1.0 / 3.0)], [(0, -2.0 / 7.0)], [(0, 0.0)]]), 1, "one group of three"),
    }


def items_call(ctx, items, m, n_items=None):
    return lib().ebcc_hip_time_map_items(ctx.ptr, items.ptr, items.shape[0] if n_items is None else n_items, ctypes.byref(m.c))


@pytest.mark.parametrize("h,w", [(37, 53), (64, 96), (90, 131)])          # (a tail of 1 pixel; none; a tail of 2 and more than one workgroup)
@pytest.mark.parametrize("base", [0, 1])
def test_kernel_against_numpy(h, w, base):
    x12 = kernel_items(h, w)
    assert (h * w) % 4 == {37: 1, 64: 0, 90: 2}[h]
    assert rule_is_visible(x12, dense_map(5, 12))
    with L.Context(4, 64, 96) as ctx:                                # (any context of the device)
        for what, (terms, n, _) in kernel_maps().items():
            x = x12[:n]
            items = R.Guarded(x, base)
            m = Map(terms, h, w, base=base).init(ctx)
            assert m.get() == np.zeros((m.n_out, h, w)).tobytes() and not m.count.any()      # (+0.0 everywhere)
            assert items_call(ctx, items, m) == 0, last_error()
            got = m.get()
            assert got == expected(x, terms).tobytes(), (what, h, w, base)
            assert m.count.tobytes() == counts(terms).tobytes()
            assert m.acc.sentinels_intact() and items.untouched()
            again = Map(terms, h, w, base=base).init(ctx)            # a second run: the same bytes
            assert items_call(ctx, items, again) == 0
            assert again.get() == got
            # without init the call adds to what the accumulators hold, and an output without terms keeps its junk
            junk = Map(terms, h, w, base=base)
            assert items_call(ctx, items, junk) == 0, last_error()
            assert junk.get() == expected(x, terms, init=JUNK).tobytes(), (what, "junk")
            assert junk.count.tobytes() == (counts(terms) + np.uint64(77)).tobytes()


def test_a_group_gives_the_bytes_of_its_outputs_alone():
    """outputs folded together and the same outputs one at a time (every other output of the dense map: nothing to join)"""
    h, w = 37, 53
    x = kernel_items(h, w)
    full = dense_map(8, 12)
    with L.Context(4, 64, 96) as ctx:
        items = R.Guarded(x, 1)
        m = Map(full, h, w).init(ctx)
        assert items_call(ctx, items, m) == 0, last_error()
        together = m.acc.get()
        for keep in (0, 1):
            rows = [[(k, weight_of(o, k)) for k in range(12)] if o % 2 == keep else [] for o in range(8)]
            alone = Map(terms_of(rows), h, w).init(ctx)
            assert items_call(ctx, items, alone) == 0, last_error()
            assert alone.acc.get()[keep::2].tobytes() == together[keep::2].tobytes()


def test_kernel_results_do_not_depend_on_alignment():
    x = kernel_items(37, 53)
    terms = kernel_maps()["mixed"][0]
    with L.Context(4, 64, 96) as ctx:
        seen = set()
        for item_base in range(4):
            for base in (0, 1):
                m = Map(terms, 37, 53, base=base).init(ctx)
                assert items_call(ctx, R.Guarded(x, item_base), m) == 0
                seen.add(m.get())
        assert len(seen) == 1


def long_lists():
    """items of 1 x 5 pixels; lists of more than 65536 entries in one call, for either launch loop"""
    def make():
        r = np.random.default_rng(65536)
        x = np.stack([(r.standard_normal((1, 5)) * 3 + 5).astype(np.float32) * R.SCALES[k % 3] for k in range(256)])
        # 300 outputs over 256 items, output o without item o % 256: no two neighbours name the same items - 76500 entries of width 1
        apart = terms_of([[(k, weight_of(o % 7, k)) for k in range(256) if k != o % 256] for o in range(300)])
        # its twin with every term: 75 groups of four, 19200 entries
        twin = terms_of([[(k, weight_of(o % 7, k)) for k in range(256)] for o in range(300)])
        # and 1100 such outputs: 275 groups, 70400 entries - the groups' launch loop passes its limit too
        wide = terms_of([[(k, weight_of(o % 7, k)) for k in range(256)] for o in range(1100)])
        return x, {"apart": (apart, expected(x, apart)), "twin": (twin, expected(x, twin)), "wide": (wide, expected(x, wide))}
    return HB.once("time map long lists", make)


@pytest.mark.parametrize("which", ["apart", "twin", "wide"])
def test_lists_longer_than_a_launch(which):
    x, maps = long_lists()
    terms, want = maps[which]
    assert {"apart": 76500, "twin": 76800, "wide": 281600}[which] == int(terms[0][-1])
    with L.Context(4, 64, 96) as ctx:
        items = R.Guarded(x, 1)
        m = Map(terms, 1, 5).init(ctx)
        assert items_call(ctx, items, m) == 0, last_error()
        assert m.get() == want.tobytes()
        assert m.count.tobytes() == counts(terms).tobytes() and m.acc.sentinels_intact() and items.untouched()


def test_kernel_refusals_write_nothing():
    x = kernel_items(37, 53)
    ok = dense_map(5, 12)
    with L.Context(4, 64, 96) as ctx:
        items = R.Guarded(x, 0)
        m = Map(ok, 37, 53).init(ctx)
        before = m.snapshot()
        nan_w = (ok[0], ok[1], ok[2].copy())
        nan_w[2][17] = np.inf
        for bad in (dense_map(5, 13),                                                       # an item >= n_items
                    terms_of([[(1, 0.5), (1, 0.5)]] + [[(0, 1.0)]] * 4),                    # an item twice in an output
                    terms_of([[(2, 0.5), (1, 0.5)]] + [[(0, 1.0)]] * 4),                    # out of order
                    terms_of([[]] * 5),                                                     # no term at all
                    nan_w):                                                                 # a weight that is not finite
            assert items_call(ctx, items, m.with_terms(bad)) == 1 and "ebcc_hip_time_map_items" in last_error()
        assert lib().ebcc_hip_time_map_items(ctx.ptr, items.ptr + 2, 12, ctypes.byref(m.c)) == 1    # items not 4-byte aligned
        assert lib().ebcc_hip_time_map_items(ctx.ptr, None, 12, ctypes.byref(m.c)) == 1
        assert lib().ebcc_hip_time_map_items(ctx.ptr, items.ptr, 12, None) == 1
        odd = m.with_terms(ok)
        odd.c.d_acc = m.acc.ptr + 4                                                         # accumulators not 8-byte aligned
        assert items_call(ctx, items, odd) == 1 and last_error()
        assert m.snapshot() == before and items.untouched()
        assert items_call(ctx, items, m) == 0, last_error()                                 # and the map still works
        assert m.get() == expected(x, ok).tobytes()


# ---- 2. streams against the oracle, across batches ---------------------------------------------------------------------------
def series8():
    streams, fields = R.series(H, W, 12)
    return list(streams[:8]), fields[:8]


def project(ctx, streams, m, row0=0, col0=0):
    keep, ptrs, sizes = R._args(streams)
    return lib().ebcc_hip_project_shard(ctx.ptr, ptrs, sizes, len(streams), row0, col0, ctypes.byref(m.c))


def stream_maps():
    return {"dense 5": dense_map(5, 8), "dense 5, one term less": dense_map(5, 8, leave={(2, 4)}), "banded": banded_map(8, 3),
            "trend-like": terms_of([[(k, 1.0 / 8.0) for k in range(8)], [(k, (k - 3.5) / 42.0) for k in range(8)]])}


def test_streams_against_the_oracle_across_batches(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series8()
    assert rule_is_visible(fields, dense_map(5, 8))
    for what, terms in stream_maps().items():
        want = expected(fields, terms).tobytes()
        seen = []
        for cap in (3, 8, 3):                                       # three batches on two engine sets; one batch; the first again
            with L.Context(cap, H, W) as ctx:
                m = Map(terms, H, W, base=1).init(ctx)
                assert project(ctx, streams, m) == 0, last_error()
                assert m.get() == want, (what, cap)
                assert m.count.tobytes() == counts(terms).tobytes() and m.acc.sentinels_intact()
                seen.append(m.get())
        assert seen[0] == seen[1] == seen[2]


def test_streams_equal_the_kernel_on_the_decoded_frames(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series8()
    terms = stream_maps()["dense 5, one term less"]
    with L.Context(3, H, W) as ctx:
        a, b = Map(terms, H, W).init(ctx), Map(terms, H, W).init(ctx)
        assert project(ctx, streams, a) == 0, last_error()
        assert items_call(ctx, R.Guarded(fields, 1), b) == 0, last_error()
        assert a.get() == b.get()


# ---- 3. a window ---------------------------------------------------------------------------------------------------------
def test_window_against_the_whole_frame(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series8()
    row0, col0, rows, cols = 9, 50, 40, 30                          # (crosses the code-block boundary at column 64)
    terms = dense_map(5, 8)
    crop = np.ascontiguousarray(fields[:, row0:row0 + rows, col0:col0 + cols])
    assert rule_is_visible(crop, terms)
    with L.Context(3, H, W) as ctx:
        win = Map(terms, rows, cols).init(ctx)
        assert project(ctx, streams, win, row0, col0) == 0, last_error()
        assert win.get() == expected(crop, terms).tobytes() and win.acc.sentinels_intact()
        whole = Map(terms, H, W).init(ctx)
        assert project(ctx, streams, whole) == 0, last_error()
        assert np.ascontiguousarray(whole.acc.get()[:, row0:row0 + rows, col0:col0 + cols]).tobytes() == win.get()


# ---- 4. unnamed frames -----------------------------------------------------------------------------------------------------
def test_unnamed_frames_are_not_read(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series8()
    named = [0, 2, 3, 5, 7]
    terms = terms_of([[(k, weight_of(o, k)) for k in named] for o in range(3)] + [[(2, 0.1), (7, -0.3)]])
    given = [s if f in named else None for f, s in enumerate(streams)]
    assert rule_is_visible(fields, terms)
    with L.Context(3, H, W) as ctx:                                 # (five named frames: two batches)
        m = Map(terms, H, W).init(ctx)
        assert project(ctx, given, m) == 0, last_error()
        assert m.get() == expected(fields, terms).tobytes() and m.count.tolist() == [5, 5, 5, 2]


# ---- 5. continuation -------------------------------------------------------------------------------------------------------
def test_a_series_split_over_two_calls(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series8()
    with L.Context(3, H, W) as ctx:
        for what, terms in stream_maps().items():
            assert what == "trend-like" or rule_is_visible(fields, terms)
            m = Map(terms, H, W).init(ctx)
            assert project(ctx, streams[:5], m.with_terms(rebased(terms, 0, 5))) == 0, last_error()
            assert m.count.tobytes() == counts(rebased(terms, 0, 5)).tobytes()
            assert project(ctx, streams[5:], m.with_terms(rebased(terms, 5, 8))) == 0, last_error()
            assert m.get() == expected(fields, terms).tobytes(), what
            assert m.count.tobytes() == counts(terms).tobytes()


# ---- 6. refusals on the device ---------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series8()
    terms = dense_map(5, 8)
    with L.Context(3, 90, 131) as other:                            # a context of another geometry
        m = Map(terms, H, W).init(other)
        before = m.snapshot()
        assert project(other, streams, m) == 1 and last_error()
        assert m.snapshot() == before
    with L.Context(3, H, W) as ctx:
        m = Map(terms, H, W).init(ctx)
        before = m.snapshot()
        bad = list(streams)
        bad[7] = bad[7][:40]                                        # a truncated header, in the last batch
        assert project(ctx, bad, m) == 1 and "ebcc_hip_project_shard" in last_error()
        assert m.snapshot() == before
        assert project(ctx, streams, m, row0=1) == 1 and last_error()                       # the window leaves the frame
        assert project(ctx, streams[:7], m) == 1 and last_error()                           # a term names frame 7 of 7
        assert project(ctx, [None] + streams[1:], m) == 1 and last_error()                  # a named frame without a stream
        assert m.snapshot() == before
        assert project(ctx, streams, m) == 0, last_error()                                  # and the context still works
        assert m.get() == expected(fields, terms).tobytes()


def test_a_stream_damaged_inside_a_later_batch(monkeypatch):
    """The damaged stream of tests/test_reduce_gpu.py: its frame header parses, the decode of its batch refuses it.  The call
    returns 1, nothing outside the accumulators is written, count stays, and the next call on the context is correct."""
    HB.use_env(monkeypatch, {})
    streams, fields = series8()

    def make():
        with L.Context(4, H, W) as ctx:
            return ctx.encode_frames(L.era5_like(H, W, 64)[None], L.make_config((1, H, W), base_cr=10, residual_type=L.NONE))[0][:40]
    damaged = HB.once("reduce damaged stream", make)
    terms = dense_map(5, 8)
    for cap, at in ((3, 4), (3, 7), (2, 5)):                        # batch 1 of three, batch 2 of three, batch 2 of four
        bad = list(streams)
        bad[at] = damaged
        with L.Context(cap, H, W) as ctx:
            m = Map(terms, H, W, base=1).init(ctx)
            assert project(ctx, bad, m) == 1 and last_error()
            assert m.acc.sentinels_intact() and not m.count.any()
            m.init(ctx)
            assert project(ctx, streams, m) == 0, last_error()
            assert m.get() == expected(fields, terms).tobytes(), (cap, at)
            assert m.acc.sentinels_intact()


# ---- 7. Python ---------------------------------------------------------------------------------------------------------------
def test_python_project_with_first_and_a_state(monkeypatch):
    HB.use_env(monkeypatch, {})
    from ebcc_amd import h5_batch
    streams, fields = series8()
    dense = np.array([[weight_of(o, k) for k in range(8)] for o in range(5)])
    dense[2, 4] = 0.0                                               # (dropped: output 2 then breaks its group)
    terms = h5_batch.time_map_terms(dense)
    assert terms[0].tolist() == [0, 8, 16, 23, 31, 39]
    want = expected(fields, terms)
    assert rule_is_visible(fields, terms)
    with h5_batch.BatchCodec(H, W, max_frames=3) as codec:
        one = codec.project(streams, dense)
        assert one.values.dtype == np.float64 and one.values.shape == (5, H, W) and one.values.tobytes() == want.tobytes()
        assert one.count.tolist() == [8, 8, 7, 8, 8]
        assert codec.project(streams, terms).values.tobytes() == want.tobytes()          # (the triple, used as given)
        with codec.map_state(5) as state:                             # the series walked in two calls
            assert codec.project(streams[:5], dense, state=state) is state
            assert state.count.tolist() == [5, 5, 4, 5, 5]
            codec.project(streams[5:], dense, state=state, first=5)
            got = state.result()
            assert got.values.tobytes() == want.tobytes() and got.count.tolist() == [8, 8, 7, 8, 8]
        win = (9, 50, 40, 30)
        crop = np.ascontiguousarray(fields[:, 9:49, 50:80])
        assert codec.project(streams, dense, window=win).values.tobytes() == expected(crop, terms).tobytes()
        trend = h5_batch.trend_weights(np.arange(8.0))
        got = codec.project(streams, trend)
        assert got.values.tobytes() == expected(fields, h5_batch.time_map_terms(trend)).tobytes()
        sparse = (np.array([0, 2, 2]), np.array([1, 6]), np.array([0.5, -0.25]))
        got = codec.project([None, streams[1], None, None, None, None, streams[6], None], sparse)
        assert got.values.tobytes() == expected(fields, h5_batch.time_map_terms(sparse)).tobytes() and got.count.tolist() == [2, 0]
        for bad in (dict(weights=np.zeros((5, 8))), dict(weights=dense, first=8), dict(weights=np.full((1, 8), np.inf)),
                    dict(weights=dense, window=(0, 0, H + 1, W))):
            with pytest.raises(ValueError):
                codec.project(streams, **bad)
        with codec.map_state(4) as state, pytest.raises(ValueError):
            codec.project(streams, dense, state=state)               # (five outputs into a state of four)
        assert codec.project(streams[:7], dense).count.tolist() == [7, 7, 6, 7, 7]      # (the terms of frame 7 belong to another call)
        with pytest.raises(RuntimeError):
            codec.project(streams[:7] + [streams[7][:40]], dense)    # a truncated stream


def test_project_frames_of_a_dataset(tmp_path):
    """h5_batch.project_frames under an interpreter with h5py, as tests/test_reduce_gpu.py drives reduce_frames"""
    if not os.path.exists(T.CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([T.CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([T.CONDA_PY, os.path.join(L.ROOT, "tests", "h5_project.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 4, r.stdout
