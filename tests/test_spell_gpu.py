"""GPU: the spell decode of include/ebcc_hip.h - ebcc_hip_spell_fold (k_spell_fold alone) and ebcc_hip_spell_shard against a plain
numpy loop over the steps in increasing index that states the rule (rule_step below):

    e = x < threshold if below else x > threshold                          (float32; a NaN is no event and ends a run)
    if fresh: run = 0;  run = run + 1 if e else 0
    if run > longest: longest = run; longest_end = when
    if run == min_len: spells += 1; spell_steps += min_len   elif run > min_len: spell_steps += 1
    if e: events += 1; first = when if first == NO_STEP; last = when
    if x > max: max = x; when_max = when     if x < min: min = x; when_min = when       (+0 is written for -0)

on numpy's own arrays (kernel alone) or on the oracle's decode of the same streams.  Everything is compared by tobytes(): there
is no tolerance in this file.  Every test that relies on its inputs first asserts about its own expected arrays that the rule
is visible in them: the backward fold, >= for the event, latest-wins on ties and an ignored `fresh` each give other bytes.

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
from tests.test_reduce_gpu import Guarded, _args

pytestmark = pytest.mark.gpu

NO_BIN = R.NO_BIN
NO_STEP = 0xFFFFFFFF
H, W = R.H, R.W
RUNS = ("d_run", "d_longest", "d_longest_end", "d_spells", "d_spell_steps")
EVENTS = ("d_events", "d_first", "d_last")
EXTREMES = ("d_min", "d_max", "d_when_min", "d_when_max")
FAMILIES = {"runs": RUNS, "events": EVENTS, "extremes": EXTREMES}
NAMES = RUNS + EVENTS + EXTREMES
FIELDS = tuple((name, np.float32 if name in ("d_min", "d_max") else np.uint32) for name in NAMES)
LABELS = ("d_longest_end", "d_first", "d_last", "d_when_min", "d_when_max")
THRESHOLD = 5.0                                        # (kernel items: N(5, 3) samples, and the value itself is planted)
STREAM_THRESHOLD = 280.0                               # (the series: a wave of amplitude 12 around 280)
MIN_LEN = 2


class SpellStats(ctypes.Structure):
    """ebcc_hip_spell_stats"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("threshold", ctypes.c_float), ("below", ctypes.c_int), ("min_len", ctypes.c_uint32)] + \
               [(name, ctypes.c_void_p) for name in NAMES] + [("count", ctypes.c_void_p)]


def lib():
    """the product with the spell entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = R.lib()
    p.ebcc_hip_spell_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(SpellStats)]
    p.ebcc_hip_spell_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.POINTER(SpellStats)]
    p.ebcc_hip_spell_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(SpellStats)]
    for name in ("ebcc_hip_spell_stats_init", "ebcc_hip_spell_fold", "ebcc_hip_spell_shard"):
        getattr(p, name).restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


last_error = R.last_error
same = R.same


class Stats:
    """the accumulators [n_bins][rows][cols] on the device, every array between sentinels, `base` words behind a 256-byte
    boundary; `leave`: names left NULL.  Filled with junk until init()."""

    def __init__(self, n_bins, rows, cols, threshold=THRESHOLD, below=0, min_len=MIN_LEN, leave=(), base=0):
        self.shape = (n_bins, rows, cols)
        self.count = np.full(n_bins, 77, np.uint64)
        self.arrays = {name: Guarded(np.full(self.shape, 3, dtype), base) for name, dtype in FIELDS if name not in leave}
        self.c = SpellStats(n_bins, rows, cols, threshold, below, min_len)
        self.c.count = self.count.ctypes.data
        for name, g in self.arrays.items():
            setattr(self.c, name, g.ptr)

    def init(self, ctx):
        assert lib().ebcc_hip_spell_stats_init(ctx.ptr, ctypes.byref(self.c)) == 0, last_error()
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


# ---- the rule, in numpy ----------------------------------------------------------------------------------------------------------
def rule_start(n_bins, rows, cols, track=True):
    """what ebcc_hip_spell_stats_init writes"""
    shape = (n_bins, rows, cols)
    s = {name: np.full(shape, NO_STEP if name in LABELS else 0, np.uint32) for name in NAMES if name not in ("d_min", "d_max")}
    s["d_min"], s["d_max"] = np.full(shape, np.inf, np.float32), np.full(shape, -np.inf, np.float32)
    s["count"] = np.zeros(n_bins, np.uint64)
    s["seen"] = set() if track else None                            # (not an accumulator: the values `run` took)
    return s


def rule_step(s, x, k, when, fresh, threshold, below, min_len, event="strict", ties="earliest", use_fresh=True):
    """one step of bin k folded into the state s; event / ties / use_fresh: the defects a kernel might have instead"""
    x, t, w = np.asarray(x, np.float32), np.float32(threshold), np.uint32(when)
    with np.errstate(invalid="ignore"):
        if event == "strict":
            e = x < t if below else x > t
        else:
            e = x <= t if below else x >= t
        run = s["d_run"][k]
        if fresh and use_fresh:
            run = np.zeros_like(run)
        run = np.where(e, run + np.uint32(1), np.uint32(0)).astype(np.uint32)
        s["d_run"][k] = run
        if s["seen"] is not None:
            s["seen"].update(np.unique(run).tolist())
        up = run > s["d_longest"][k] if ties == "earliest" else (run >= s["d_longest"][k]) & (run > 0)
        s["d_longest"][k] = np.where(up, run, s["d_longest"][k])
        s["d_longest_end"][k] = np.where(up, w, s["d_longest_end"][k])
        s["d_spells"][k] += run == min_len
        s["d_spell_steps"][k] += np.where(run == min_len, np.uint32(min_len), np.uint32(0)) + (run > min_len)
        s["d_events"][k] += e
        s["d_first"][k] = np.where(e & (s["d_first"][k] == NO_STEP), w, s["d_first"][k])
        s["d_last"][k] = np.where(e, w, s["d_last"][k])
        hi = x > s["d_max"][k] if ties == "earliest" else x >= s["d_max"][k]
        s["d_max"][k] = np.where(hi, x, s["d_max"][k])
        s["d_when_max"][k] = np.where(hi, w, s["d_when_max"][k])
        lo = x < s["d_min"][k] if ties == "earliest" else x <= s["d_min"][k]
        s["d_min"][k] = np.where(lo, x, s["d_min"][k])
        s["d_when_min"][k] = np.where(lo, w, s["d_when_min"][k])
    s["count"][k] += 1


def rule_bytes(s):
    out = {name: (s[name] + np.float32(0.0) if name in ("d_min", "d_max") else s[name]).tobytes() for name in NAMES}      # (-0 -> +0)
    out["count"] = s["count"].tobytes()
    return out


def rule_fold(s, fields, bins=None, when=None, fresh=None, threshold=THRESHOLD, below=0, min_len=MIN_LEN, order=None, first_label=0, **defect):
    for t in (range(len(fields)) if order is None else order):
        k = 0 if bins is None else int(bins[t])
        if k == NO_BIN:
            continue
        rule_step(s, fields[t], k, first_label + t if when is None else when[t], bool(fresh is not None and fresh[t]), threshold, below, min_len, **defect)
    return s


def expected(fields, bins, n_bins, when=None, fresh=None, threshold=THRESHOLD, below=0, min_len=MIN_LEN, order=None, seen=None, **defect):
    """the loop the header states, on `fields` [n][rows][cols] float32 -> {name: bytes}; order: the steps' order (None: increasing)"""
    fields = np.asarray(fields, np.float32)
    s = rule_fold(rule_start(n_bins, *fields.shape[1:]), fields, bins, when, fresh, threshold, below, min_len, order, **defect)
    if seen is not None:
        seen.update(s["seen"])
    return rule_bytes(s)


def the_rule_is_visible(fields, bins, n_bins, when, fresh, threshold=THRESHOLD, below=0, min_len=MIN_LEN, with_fresh=True, planted=True):
    """about the expected arrays themselves: a wrong order, a wrong comparison, a wrong tie rule or an ignored flag cannot pass.
    planted=False: decoded fields, in which no sample is known to equal the threshold or another step's sample - the order, the
    run lengths and the ties of the longest runs are still asserted"""
    kw = dict(when=when, fresh=fresh, threshold=threshold, below=below, min_len=min_len)
    seen = set()
    fwd = expected(fields, bins, n_bins, seen=seen, **kw)
    rev = expected(fields, bins, n_bins, order=range(len(fields) - 1, -1, -1), **kw)
    assert all(fwd[name] != rev[name] for name in ("d_longest_end", "d_first", "d_last", "d_run")) and fwd["d_events"] == rev["d_events"]
    late = expected(fields, bins, n_bins, ties="latest", **kw)
    assert fwd["d_longest_end"] != late["d_longest_end"] and fwd["d_longest"] == late["d_longest"]
    if planted:
        assert fwd["d_events"] != expected(fields, bins, n_bins, event="inclusive", **kw)["d_events"]
        assert fwd["d_when_max"] != late["d_when_max"]
    if with_fresh:
        assert fwd["d_longest"] != expected(fields, bins, n_bins, use_fresh=False, **kw)["d_longest"]
    # runs shorter than, equal to and longer than min_len: `run` took the values 0, 1, min_len and more, and somewhere the
    # longest run of all is 1
    assert {0, 1, min_len} <= seen and max(seen) > min_len > 1
    assert not planted or (np.frombuffer(fwd["d_longest"], np.uint32) == 1).any()
    spells, steps = np.frombuffer(fwd["d_spells"], np.uint32), np.frombuffer(fwd["d_spell_steps"], np.uint32)
    assert (spells > 0).any() and (steps > spells * min_len).any()
    return True


# ---- 1. the kernel alone against numpy ---------------------------------------------------------------------------------------
KERNEL_BINS = [0, 1, NO_BIN, 0, 2, 1, 0]               # three bins, a bin left and come back to, a skipped item; bin 3 of 4 is never named
KERNEL_WHEN = [40, 10, 99, 30, 20, 5, 50]              # (not monotone)
KERNEL_FRESH = [0, 0, 0, 0, 0, 1, 0]                   # item 5: the second of bin 1 - inside a run wherever items 1 and 5 are both events
N_ITEMS = len(KERNEL_BINS)


def kernel_items(h, w):
    """seven items of N(5, 3) samples; item 6 repeats item 0 (ties at every pixel: both lie in bin 0), the threshold itself, a
    NaN, -0 and +0 are planted"""
    def make():
        r = np.random.default_rng(h * 1000 + w)
        x = (r.standard_normal((N_ITEMS, h, w)) * 3 + 5).astype(np.float32)
        x[6] = x[0]
        x[0, 0, 0] = x[3, h - 1, w - 1] = x[1, 0, 2] = THRESHOLD  # (x == threshold is no event, whichever way `below` points)
        x[6, 0, 0] = THRESHOLD
        x[1, 0, 1] = x[5, 0, 1] = -0.0                              # bin 1: min and max are -0 -> +0 is written
        x[3, 1, 0] = np.nan                                         # bin 0: a NaN between items 0 and 6 - no event, not an extreme
        x[0, 1, 0] = x[6, 1, 0] = 9.0
        x.setflags(write=False)
        return x
    return HB.once(("spell kernel items", h, w), make)


def layout(what):
    return (KERNEL_BINS, 4, KERNEL_WHEN, KERNEL_FRESH) if what == "bins" else (None, 1, None, [0, 0, 0, 0, 1, 0, 0])


def kernel_want(h, w, what, below):
    bins, n_bins, when, fresh = layout(what)
    return HB.once(("spell kernel want", h, w, what, below), lambda: expected(kernel_items(h, w), bins, n_bins, when, fresh, below=below))


def fold(ctx, items, bins, when, fresh, stats, n=None):
    b = None if bins is None else np.asarray(bins, np.uint32)
    t = None if when is None else np.asarray(when, np.uint32)
    f = None if fresh is None else np.asarray(fresh, np.uint8)
    return lib().ebcc_hip_spell_fold(ctx.ptr, items.ptr, items.shape[0] if n is None else n, None if b is None else b.ctypes.data,
                                     None if t is None else t.ctypes.data, None if f is None else f.ctypes.data, ctypes.byref(stats.c))


@pytest.mark.parametrize("h,w", [(37, 53), (64, 96), (90, 131)])          # (a tail of 1 pixel; none; a tail of 2 and more than one workgroup)
@pytest.mark.parametrize("base", [0, 1])
def test_kernel_against_numpy(h, w, base):
    x = kernel_items(h, w)
    assert (h * w) % 4 == {37: 1, 64: 0, 90: 2}[h]
    start = rule_bytes(rule_start(4, h, w))
    with L.Context(4, 64, 96) as ctx:                                # (any context of the device)
        items = Guarded(x, base)
        assert (items.ptr % 16 == 0) == (base == 0)                  # (both load paths)
        for below in (0, 1):
            for what in ("bins", "no list"):
                bins, n_bins, when, fresh = layout(what)
                assert the_rule_is_visible(x, bins, n_bins, when, fresh, below=below)
                want = kernel_want(h, w, what, below)
                st = Stats(n_bins, h, w, below=below, base=base).init(ctx)
                if n_bins == 4:                                       # (the initial values, which bin 3 keeps)
                    same(st.get(), start, "init")
                assert fold(ctx, items, bins, when, fresh, st) == 0, last_error()
                got = st.get()
                same(got, want, (what, h, w, base, below))
                if n_bins == 4:
                    assert np.frombuffer(got["count"], np.uint64).tolist() == [3, 2, 1, 0]
                    for name, dtype in FIELDS:
                        assert st.arrays[name].get()[3].tobytes() == np.frombuffer(start[name], dtype).reshape(st.shape)[3].tobytes()
                    mn, mx = (np.frombuffer(got[name], np.float32).reshape(4, h, w) for name in ("d_min", "d_max"))
                    zero = np.float32(0.0).tobytes()
                    assert mn[1, 0, 1].tobytes() == zero and mx[1, 0, 1].tobytes() == zero                  # (-0 leaves as +0)
                    run = np.frombuffer(got["d_run"], np.uint32).reshape(4, h, w)
                    assert run[0, 1, 0] == (0 if below else 1) and run[0, 0, 0] == 0                        # (the NaN ended the run; x == threshold)
                assert st.sentinels_intact() and items.untouched()
                again = Stats(n_bins, h, w, below=below, base=base).init(ctx)                               # a second run: the same bytes
                assert fold(ctx, items, bins, when, fresh, again) == 0
                assert again.get() == got


# ---- 2. accumulators left NULL -----------------------------------------------------------------------------------------------
SUBSETS = [("runs",), ("events",), ("extremes",), ("runs", "events"), ("runs", "extremes"), ("events", "extremes")]


@pytest.mark.parametrize("kept", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_kernel_with_accumulators_left_null(kept):
    h, w = 37, 53
    x = kernel_items(h, w)
    full = kernel_want(h, w, "bins", 0)
    names = sum((FAMILIES[f] for f in kept), ())
    want = {name: full[name] for name in names + ("count",)}
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 1)
        st = Stats(4, h, w, leave=[name for name in NAMES if name not in names]).init(ctx)
        assert fold(ctx, items, KERNEL_BINS, KERNEL_WHEN, KERNEL_FRESH, st) == 0, last_error()
        got = st.get()
        assert sorted(got) == sorted(want)
        same(got, want, kept)
        assert st.sentinels_intact() and items.untouched()
        # within a family: the arrays that need no other one, each alone
        for name in ("d_run", "d_events", "d_first", "d_last", "d_min", "d_max"):
            one = Stats(4, h, w, leave=[n for n in NAMES if n != name]).init(ctx)
            assert fold(ctx, items, KERNEL_BINS, KERNEL_WHEN, KERNEL_FRESH, one) == 0, last_error()
            assert one.get()[name] == full[name] and one.sentinels_intact(), name


# ---- 3. a list longer than one launch ------------------------------------------------------------------------------------------
def test_a_list_longer_than_one_launch():
    cut, n = 65536, 65536 + 5
    r = np.random.default_rng(5)
    x = (r.standard_normal((n, 1, 7)) * 3 + 5).astype(np.float32)
    x[cut - 30:, 0, :4] = 9.0                                         # pixels 0..3: a run of 35 events across the launch boundary, the longest
    x[cut - 31, 0, :4] = 1.0
    when = ((np.arange(n, dtype=np.uint64) * 7919) % 100003).astype(np.uint32)
    head = rule_fold(rule_start(1, 1, 7, track=False), x[:cut], None, when[:cut])

    def tail(fresh):
        s = {name: (None if name == "seen" else v.copy()) for name, v in head.items()}
        return rule_bytes(rule_fold(s, x[cut:], None, when[cut:], fresh))
    assert (head["d_run"][0, 0, :4] == 30).all()
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 1)
        wants = {}
        for what, flag in (("no flag", 0), ("a flag on the first entry of the second launch", 1)):
            fresh = np.zeros(n, np.uint8)
            fresh[cut] = flag
            want = wants[what] = tail(fresh[cut:])
            st = Stats(1, 1, 7, base=1).init(ctx)
            assert fold(ctx, items, None, when, fresh, st) == 0, last_error()
            same(st.get(), want, what)
            assert np.frombuffer(want["d_run"], np.uint32)[:4].tolist() == [5 if flag else 35] * 4
            assert np.frombuffer(want["d_longest"], np.uint32)[:4].tolist() == [30 if flag else 35] * 4
            assert st.sentinels_intact() and items.untouched()
        assert wants["no flag"]["d_longest"] != wants["a flag on the first entry of the second launch"]["d_longest"]


# ---- 4. refusals of the kernel call ----------------------------------------------------------------------------------------------
def test_kernel_refusals_write_nothing():
    x = kernel_items(37, 53)
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 0)
        st = Stats(4, 37, 53).init(ctx)
        before = st.snapshot()
        f = lib().ebcc_hip_spell_fold
        call = lambda bins=KERNEL_BINS, when=KERNEL_WHEN: fold(ctx, items, bins, when, KERNEL_FRESH, st)      # noqa: E731
        assert call(bins=[0, 1, 4, 0, 2, 1, 0]) == 1 and "ebcc_hip_spell_fold" in last_error()               # a bin >= n_bins
        assert call(bins=[NO_BIN] * N_ITEMS) == 1 and last_error()                                           # no item named
        assert call(when=[40, 10, 99, NO_STEP, 20, 5, 50]) == 1 and "label" in last_error()                  # a named item with the label NO_STEP
        assert f(ctx.ptr, items.ptr + 2, N_ITEMS, None, None, None, ctypes.byref(st.c)) == 1 and last_error()   # items not 4-byte aligned
        assert f(ctx.ptr, None, N_ITEMS, None, None, None, ctypes.byref(st.c)) == 1 and last_error()
        assert f(ctx.ptr, items.ptr, N_ITEMS, None, None, None, None) == 1 and last_error()
        st.c.threshold = float("nan")
        assert call() == 1 and "threshold" in last_error()
        st.c.threshold = THRESHOLD
        st.c.min_len = 0
        assert call() == 1 and "min_len" in last_error()
        st.c.min_len = MIN_LEN
        for name, needs in (("d_run", "d_run"), ("d_longest", "d_longest"), ("d_max", "d_max"), ("d_min", "d_min")):
            keep = getattr(st.c, name)
            setattr(st.c, name, None)
            assert call() == 1 and needs in last_error(), name
            setattr(st.c, name, keep)
        st.c.d_first += 2
        assert call() == 1 and "4-byte" in last_error()
        st.c.d_first -= 2
        assert st.snapshot() == before and items.untouched()
        assert call() == 0, last_error()                                                                     # and the call still works
        same(st.get(), kernel_want(37, 53, "bins", 0), "after refusals")


# ---- 5. streams against the oracle, across batches ---------------------------------------------------------------------------
N_STEPS = 16
MOVES = [0, 24, 24, 3, 3, 24, 3, 3, 3, 24, 24, 24, 3, 3, 3, 3]            # columns the wave moves before each step (24: half a period)
ONE_BIN = [0] * N_STEPS
BINS16 = [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 2, 0, 0]                 # bins 0 and 1 are come back to; bin 2 has one step
WHEN16 = [300 + 7 * t if t % 2 else 200 - t for t in range(N_STEPS)]      # (not monotone)
FRESH16 = [1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0]                # the first step of every visit - but not of the last (steps 14, 15)


def spell_series(h, w, n):
    """n frames of one scale - a wave of amplitude 12 around 280 whose crossing of 280 moves across the frame from step to step,
    with a little noise -, their streams from the product's encode and the oracle's decode of those streams; made once"""
    def make():
        L.oracle().orc_set_j2k_backend(0)
        row, col = np.mgrid[0:h, 0:w]
        shift = np.cumsum(MOVES[:n])
        x = np.stack([280 + 12 * np.sin(2 * np.pi * (col - shift[t]) / 48.0 + row / 20.0) + np.random.default_rng(900 + t).normal(0, 0.3, (h, w))
                      for t in range(n)]).astype(np.float32)
        cfg = L.make_config((1, h, w), base_cr=20.0, error=0.004, residual_type=L.RELATIVE_ERROR)
        with L.Context(16, h, w) as ctx:
            streams = ctx.encode_frames(x, cfg)
        fields = np.stack([L.orc_decode(s).reshape(h, w) for s in streams])
        fields.setflags(write=False)
        return streams, fields
    return HB.once(("spell series", h, w, n), make)


STREAM_KW = dict(threshold=STREAM_THRESHOLD, min_len=MIN_LEN)
LAYOUTS = (("one bin", ONE_BIN, 1, None, None), ("bins", BINS16, 3, WHEN16, FRESH16))


def stream_want(what):
    _, bins, n_bins, when, fresh = [lay for lay in LAYOUTS if lay[0] == what][0]
    return HB.once(("spell stream want", what), lambda: expected(spell_series(H, W, N_STEPS)[1], bins, n_bins, when, fresh, **STREAM_KW))


def spell(ctx, streams, bins, when, fresh, stats, row0=0, col0=0):
    keep, ptrs, sizes = _args(streams)
    b = None if bins is None else np.asarray(bins, np.uint32)
    t = None if when is None else np.asarray(when, np.uint32)
    f = None if fresh is None else np.asarray(fresh, np.uint8)
    return lib().ebcc_hip_spell_shard(ctx.ptr, ptrs, sizes, len(streams), None if b is None else b.ctypes.data, None if t is None else t.ctypes.data,
                                      None if f is None else f.ctypes.data, row0, col0, ctypes.byref(stats.c))


def stream_stats(n_bins, rows=H, cols=W, **kw):
    return Stats(n_bins, rows, cols, STREAM_THRESHOLD, 0, MIN_LEN, **kw)


def test_streams_against_the_oracle_across_batches(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = spell_series(H, W, N_STEPS)
    # run lengths 0, 1, min_len and more occur and the longest runs tie, on the oracle-decoded fields
    assert the_rule_is_visible(fields, ONE_BIN, 1, None, None, with_fresh=False, planted=False, **STREAM_KW)
    assert the_rule_is_visible(fields, BINS16, 3, WHEN16, FRESH16, planted=False, **STREAM_KW)
    for what, bins, n_bins, when, fresh in LAYOUTS:
        want = stream_want(what)
        seen = []
        for cap in (5, 16, 5):                                      # four batches on two engine sets; one batch; the first again
            with L.Context(cap, H, W) as ctx:
                st = stream_stats(n_bins, base=1).init(ctx)
                assert spell(ctx, streams, None if what == "one bin" else bins, when, fresh, st) == 0, last_error()
                got = st.get()
                same(got, want, f"capacity {cap}, {what}")
                assert st.sentinels_intact()
                seen.append(got)
        assert seen[0] == seen[1] == seen[2]
        assert np.frombuffer(seen[0]["count"], np.uint64).tolist() == ([9, 6, 1] if n_bins == 3 else [16])


# ---- 6. the shard call equals the kernel on the decoded fields ------------------------------------------------------------------
def test_the_shard_call_equals_the_kernel_on_the_decoded_fields(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = spell_series(H, W, N_STEPS)
    with L.Context(6, H, W) as ctx:
        a = stream_stats(3).init(ctx)
        assert spell(ctx, streams, BINS16, WHEN16, FRESH16, a) == 0, last_error()
        b = stream_stats(3, base=1).init(ctx)
        assert fold(ctx, Guarded(fields, 1), BINS16, WHEN16, FRESH16, b) == 0, last_error()
        assert a.get() == b.get()


# ---- 7. a window -----------------------------------------------------------------------------------------------------------
def test_window(monkeypatch):
    HB.use_env(monkeypatch, {})
    h, w, (row0, col0, rows, cols) = 90, 131, (9, 50, 40, 30)       # (crosses the code-block boundary at column 64)
    n = 8
    streams, fields = spell_series(h, w, n)
    bins, when, fresh = BINS16[:n], WHEN16[:n], FRESH16[:n]
    crop = fields[:, row0:row0 + rows, col0:col0 + cols]
    want = expected(crop, bins, 3, when, fresh, **STREAM_KW)
    with L.Context(3, h, w) as ctx:                                 # (three batches)
        whole = stream_stats(3, h, w).init(ctx)
        assert spell(ctx, streams, bins, when, fresh, whole) == 0, last_error()
        same(whole.get(), expected(fields, bins, 3, when, fresh, **STREAM_KW), "whole frame")
        st = stream_stats(3, rows, cols, base=1).init(ctx)
        assert spell(ctx, streams, bins, when, fresh, st, row0, col0) == 0, last_error()
        got = st.get()
        for name, dtype in FIELDS:                                  # the crop of the whole-frame result
            assert got[name] == whole.arrays[name].get()[:, row0:row0 + rows, col0:col0 + cols].tobytes(), name
        same(got, want, "window")
        assert st.sentinels_intact()


# ---- 8. skipped steps -------------------------------------------------------------------------------------------------------
def test_skipped_steps_are_not_read(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = spell_series(H, W, N_STEPS)
    bins, given = list(BINS16), list(streams)
    for t in (1, 4, 7, 15):
        bins[t], given[t] = NO_BIN, None
    fresh = list(FRESH16)
    fresh[4] = 1                                                    # (the flag of a skipped step is not looked at)
    want = expected(fields, bins, 3, WHEN16, FRESH16, **STREAM_KW)
    assert want == expected(fields, bins, 3, WHEN16, fresh, **STREAM_KW) and want != stream_want("bins")
    with L.Context(5, H, W) as ctx:                                 # (twelve named steps: three batches)
        st = stream_stats(3).init(ctx)
        assert spell(ctx, given, bins, WHEN16, fresh, st) == 0, last_error()
        same(st.get(), want, "skipped")
        assert st.count.tolist() == [6, 5, 1] and st.sentinels_intact()


# ---- 9. continuation --------------------------------------------------------------------------------------------------------
def test_a_series_split_over_two_calls(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = spell_series(H, W, N_STEPS)
    cut = 8                                                          # (steps 6..9 move the wave little: most runs go on over the cut)
    before = rule_fold(rule_start(1, H, W), fields[:cut], threshold=STREAM_THRESHOLD)
    assert ((before["d_run"][0] > 0) & (fields[cut] > np.float32(STREAM_THRESHOLD))).mean() > 0.25       # the split falls inside a run
    labels = list(range(N_STEPS))
    with L.Context(5, H, W) as ctx:
        for what, bins, n_bins, when, fresh in LAYOUTS:
            when = labels if when is None else when                  # (the default labels count from 0 in every call)
            st = stream_stats(n_bins).init(ctx)
            assert spell(ctx, streams[:cut], bins[:cut], when[:cut], None if fresh is None else fresh[:cut], st) == 0, last_error()
            assert st.count.tolist() == ([5, 3, 0] if n_bins == 3 else [8])
            assert spell(ctx, streams[cut:], bins[cut:], when[cut:], None if fresh is None else fresh[cut:], st) == 0, last_error()
            same(st.get(), stream_want(what), f"two calls, {what}")
            assert st.sentinels_intact()


# ---- 10. refusals on the device ------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = spell_series(H, W, N_STEPS)
    with L.Context(5, 90, 131) as other:                            # a context of another geometry
        st = stream_stats(3).init(other)
        before = st.snapshot()
        assert spell(other, streams, BINS16, WHEN16, FRESH16, st) == 1 and last_error()
        assert st.snapshot() == before
    with L.Context(5, H, W) as ctx:
        st = stream_stats(3).init(ctx)
        assert spell(ctx, streams[:2], BINS16[:2], WHEN16[:2], FRESH16[:2], st) == 0, last_error()        # (a count that is not zero)
        assert st.count.tolist() == [2, 0, 0]
        before = st.snapshot()
        call = lambda s=streams, b=BINS16, t=WHEN16, **kw: spell(ctx, s, b, t, FRESH16, st, **kw)         # noqa: E731
        bad = list(streams)
        bad[14] = bad[14][:40]                                      # a truncated header, in the last batch
        assert call(s=bad) == 1 and "frame 14" in last_error()
        assert call(s=[None] + list(streams[1:])) == 1 and "frame 0" in last_error()                      # a named step without a stream
        assert call(row0=1) == 1 and "window" in last_error()                                            # the window leaves the frame
        assert call(b=[0, 1, 3, 0] * 4) == 1 and "bin" in last_error()                                   # a bin >= n_bins
        assert call(t=WHEN16[:9] + [NO_STEP] + WHEN16[10:]) == 1 and "step 9" in last_error()            # a named step with the label NO_STEP
        st.c.threshold = float("nan")
        assert call() == 1 and "threshold" in last_error()
        st.c.threshold = STREAM_THRESHOLD
        keep, st.c.d_run = st.c.d_run, None
        assert call() == 1 and "d_run" in last_error()
        st.c.d_run = keep
        assert lib().ebcc_hip_spell_shard(ctx.ptr, None, None, N_STEPS, None, None, None, 0, 0, ctypes.byref(st.c)) == 1 and last_error()
        assert st.snapshot() == before
        # and the context still works
        st.init(ctx)
        assert call() == 0, last_error()
        same(st.get(), stream_want("bins"), "after refusals")


# ---- 11. a stream damaged inside a later batch ---------------------------------------------------------------------------------
def test_a_stream_damaged_inside_a_later_batch(monkeypatch):
    """The damaged stream of tests/test_reduce_gpu.py: the frame header parses, the decode of its batch refuses it.  The call
    returns 1, count is what it was, nothing outside the accumulators is written, and after a new init the next call on the
    context is correct."""
    HB.use_env(monkeypatch, {})
    streams, fields = spell_series(H, W, N_STEPS)

    def make():
        with L.Context(4, H, W) as ctx:
            return ctx.encode_frames(L.era5_like(H, W, 64)[None], L.make_config((1, H, W), base_cr=10, residual_type=L.NONE))[0][:40]
    damaged = HB.once("reduce damaged stream", make)
    for cap, at in ((5, 12), (3, 7)):                               # in batch 2 of four; in batch 2 of six
        bad = list(streams)
        bad[at] = damaged
        with L.Context(cap, H, W) as ctx:
            st = stream_stats(3, base=1).init(ctx)
            assert spell(ctx, streams[:2], BINS16[:2], WHEN16[:2], FRESH16[:2], st) == 0, last_error()
            assert st.count.tolist() == [2, 0, 0]
            assert spell(ctx, bad, BINS16, WHEN16, FRESH16, st) == 1 and last_error()
            assert st.count.tolist() == [2, 0, 0] and st.sentinels_intact()
            st.init(ctx)
            assert spell(ctx, streams, BINS16, WHEN16, FRESH16, st) == 0, last_error()
            same(st.get(), stream_want("bins"), f"after the damaged stream at {at} of batches of {cap}")
            assert st.sentinels_intact()


# ---- 12. the reduce decode's bytes ---------------------------------------------------------------------------------------------
def test_min_max_and_events_are_the_reduce_decode(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = spell_series(H, W, N_STEPS)
    with L.Context(5, H, W) as ctx:
        st = stream_stats(3).init(ctx)
        assert spell(ctx, streams, BINS16, WHEN16, FRESH16, st) == 0, last_error()
        alone = R.Stats(3, H, W, threshold=STREAM_THRESHOLD).init(ctx)
        assert R.reduce(ctx, streams, BINS16, alone) == 0, last_error()
        got, ref = st.get(), alone.get()
        assert got["d_min"] == ref["d_min"] and got["d_max"] == ref["d_max"] and got["d_events"] == ref["d_over"] and got["count"] == ref["count"]
        assert 0 < np.frombuffer(ref["d_over"], np.uint32).sum() < N_STEPS * H * W
    # and the kernels alone on items with -0, +0 and a NaN
    x = kernel_items(37, 53)
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 1)
        st = Stats(4, 37, 53).init(ctx)
        assert fold(ctx, items, KERNEL_BINS, KERNEL_WHEN, KERNEL_FRESH, st) == 0, last_error()
        alone = R.Stats(4, 37, 53, threshold=THRESHOLD).init(ctx)
        assert R.fold(ctx, items, KERNEL_BINS, alone) == 0, last_error()
        got, ref = st.get(), alone.get()
        assert got["d_min"] == ref["d_min"] and got["d_max"] == ref["d_max"] and got["d_events"] == ref["d_over"]


# ---- 13. Python ------------------------------------------------------------------------------------------------------------------
def test_batch_codec_spells_with_a_state(monkeypatch):
    HB.use_env(monkeypatch, {})
    from ebcc_amd import h5_batch as B
    streams, fields = spell_series(H, W, N_STEPS)
    want = stream_want("bins")
    bins = [int(b) for b in BINS16]
    with B.BatchCodec(H, W, max_frames=5) as codec:
        with codec.spell_state(STREAM_THRESHOLD, min_len=MIN_LEN, n_bins=3) as state:
            assert codec.spells(streams[:7], None, bins=bins[:7], when=WHEN16[:7], fresh=FRESH16[:7], state=state) is state
            codec.spells(streams[7:], None, bins=bins[7:], when=WHEN16[7:], fresh=FRESH16[7:], state=state)
            got = state.result()
        one = codec.spells(streams, STREAM_THRESHOLD, min_len=MIN_LEN, bins=bins, when=WHEN16, fresh=FRESH16, n_bins=3)
        for res in (got, one):
            for name in NAMES:
                assert getattr(res, name[2:]).tobytes() == want[name], name
            assert res.count.tobytes() == want["count"]
        first = got.masked("first")
        assert first.mask.any() and not first.mask.all() and np.array_equal(first.mask, got.first == NO_STEP)
        with pytest.raises(ValueError):
            got.masked("run")
        # one family: the others are None; the default labels are the indices; below
        bare = codec.spells(streams, STREAM_THRESHOLD, below=True, what=("events",))
        assert all(getattr(bare, name[2:]) is None for name in RUNS + EXTREMES)
        cold = expected(fields, None, 1, threshold=STREAM_THRESHOLD, below=1)
        assert all(getattr(bare, name[2:]).tobytes() == cold[name] for name in EVENTS) and bare.count.tolist() == [16]
        runs0 = codec.spells(streams, STREAM_THRESHOLD, min_len=0, what="runs")                          # (min_len 0: no spells)
        assert runs0.spells is None and runs0.spell_steps is None and runs0.longest.tobytes() == stream_want("one bin")["d_longest"]
        skipped = codec.spells([None] + list(streams[1:]), STREAM_THRESHOLD, bins=[-1] + [0] * 15, what=("extremes",))
        assert skipped.count.tolist() == [15] and skipped.when_max.min() >= 1
        for bad in (dict(bins=[0] * 15), dict(bins=[-1] * 16), dict(bins=[3] * 16, n_bins=3), dict(when=[NO_STEP] * 16), dict(when=[0] * 15),
                    dict(fresh=[0] * 15), dict(what=()), dict(what=("spells",)), dict(n_bins=0), dict(window=(0, 0, H + 1, W))):
            with pytest.raises(ValueError):
                codec.spells(streams, STREAM_THRESHOLD, **bad)
        with pytest.raises(ValueError):
            codec.spells(streams, float("nan"))
        assert codec.spells(streams, float("nan"), what=("extremes",)).max.tobytes() == stream_want("one bin")["d_max"]


def test_spell_frames_of_a_dataset(tmp_path):
    """h5_batch.spell_frames under an interpreter with h5py, as tests/test_pair_gpu.py drives pair_frames"""
    from ebcc_amd import h5_batch
    assert callable(h5_batch.spell_frames)                          # (missing: a failure, not a skip)
    if not os.path.exists(T.CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([T.CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([T.CONDA_PY, os.path.join(L.ROOT, "tests", "h5_spell.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 3, r.stdout
