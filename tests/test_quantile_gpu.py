"""GPU: the quantile decode of include/ebcc_hip.h - ebcc_hip_rank_items (k_rank_count and k_rank_advance alone) and
ebcc_hip_quantile_shard against

    np.sort(fields + np.float32(0), axis=0)[rank]        with every NaN rewritten to 0x7FC00000

on numpy's own arrays (kernels alone) or on the oracle's decode of the same streams.  Everything is compared by tobytes(): there
is no tolerance in this file.

Not tested here: the refusal of a context for chunks of several frames (the reduce decode's tests leave it out too), and a
failed allocation of the workspace."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L
from tests import test_audit_gpu as A
from tests import test_reduce_gpu as R
from tests import test_window_gpu as T

pytestmark = pytest.mark.gpu

NO_BIN = 0xFFFFFFFF
NO_RANK = 2 ** 64 - 1
NAN_BITS = np.uint32(0x7FC00000)
JUNK = np.uint32(0x3C3C3C3C)                            # what d_out holds before a call
H, W = 64, 96
Guarded = R.Guarded


class TimeRanks(ctypes.Structure):
    """ebcc_hip_time_ranks"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t), ("n_ranks", ctypes.c_size_t),
                ("rank", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("count", ctypes.c_void_p)]


def lib():
    """the product with the quantile entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = R.lib()
    p.ebcc_hip_rank_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(TimeRanks)]
    p.ebcc_hip_quantile_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.POINTER(TimeRanks)]
    for name in ("ebcc_hip_rank_items", "ebcc_hip_quantile_shard"):
        getattr(p, name).restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


class Ranks:
    """a spec: the rank table [n_bins][n_ranks] on the host, d_out [n_bins][n_ranks][rows][cols] of junk on the device between
    sentinels, `base` words behind a 256-byte boundary, and a count array of 77s"""

    def __init__(self, ranks, rows, cols, base=0):
        self.table = np.ascontiguousarray(np.asarray(ranks, np.uint64).reshape(len(ranks), -1))
        self.shape = self.table.shape + (rows, cols)
        self.out = Guarded(np.full(self.shape, JUNK, np.uint32), base)
        self.count = np.full(self.table.shape[0], 77, np.uint64)
        self.c = TimeRanks(self.shape[0], rows, cols, self.shape[1], self.table.ctypes.data, self.out.ptr, self.count.ctypes.data)

    def get(self):
        return self.out.get()

    def snapshot(self):
        return self.out.all().tobytes(), self.count.tobytes()


def expected(fields, bins, ranks):
    """(the planes as uint32 [n_bins][n_ranks][rows][cols], an unused slot's left as junk; the count) by numpy's sort"""
    fields = np.asarray(fields, np.float32)
    table = np.asarray(ranks, np.uint64).reshape(len(ranks), -1)
    b = np.zeros(len(fields), np.int64) if bins is None else np.asarray(bins, np.int64)
    want = np.full(table.shape + fields.shape[1:], JUNK, np.uint32)
    count = np.zeros(table.shape[0], np.uint64)
    for k in range(table.shape[0]):
        sel = fields[b == k]
        count[k] = len(sel)
        if not len(sel):
            continue
        with np.errstate(invalid="ignore"):                          # (a signalling NaN among the samples)
            order = np.sort(sel + np.float32(0), axis=0)             # (-0 -> +0; NaN last)
        for j, r in enumerate(table[k]):
            if int(r) != NO_RANK:
                plane = order[int(r)]
                want[k, j] = np.where(np.isnan(plane), NAN_BITS, plane.view(np.uint32))
    return want, count


def rank_items(ctx, items, bins, spec, n=None):
    b = None if bins is None else np.asarray(bins, np.uint32)
    return lib().ebcc_hip_rank_items(ctx.ptr, items.ptr, items.shape[0] if n is None else n, None if b is None else b.ctypes.data, ctypes.byref(spec.c))


def same(spec, want, what):
    planes, count = want
    assert spec.get().tobytes() == planes.tobytes(), what
    assert spec.count.tobytes() == count.tobytes(), what
    assert spec.out.sentinels_intact(), what


# ---- 1. the kernels alone against numpy ----------------------------------------------------------------------------------------
KERNEL_BINS = [0, 1, 1, 0, 2]                          # a bin left and come back to, a repeat; bin 3 of 4 is never named
KERNEL_RANKS = [[0, 1, 0], [1, NO_RANK, 0], [NO_RANK, 0, NO_RANK], [NO_RANK] * 3]


@pytest.mark.parametrize("h,w", [(37, 53), (64, 96), (90, 131)])          # (a tail of 1 pixel; none; a tail of 2 and more than one workgroup)
@pytest.mark.parametrize("base", [0, 1])
def test_kernels_against_numpy(h, w, base):
    x12 = R.kernel_items(h, w, 12)
    assert (h * w) % 4 == {37: 1, 64: 0, 90: 2}[h]
    with L.Context(4, 64, 96) as ctx:                                # (any context of the device)
        # twelve items in one bin; the same rank in two slots gives two identical planes
        items = Guarded(x12, base)
        for bins in ([0] * 12, None):
            spec = Ranks([[0, 5, 11, 5]], h, w, base)
            assert rank_items(ctx, items, bins, spec) == 0, last_error()
            same(spec, expected(x12, bins, [[0, 5, 11, 5]]), ("one bin", h, w, base))
            got = spec.get()
            assert got[0, 1].tobytes() == got[0, 3].tobytes() and spec.count.tolist() == [12]
        assert items.untouched()
        # five items in three of four bins, ranks per bin; bin 3 is not named and its planes keep their junk
        x = x12[:5]
        items = Guarded(x, base)
        for bins, counts in ((KERNEL_BINS, [2, 2, 1, 0]), ([0, 1, 1, NO_BIN, 2], None)):
            ranks = KERNEL_RANKS if counts else [[0, NO_RANK, 0], [1, NO_RANK, 0], [NO_RANK, 0, NO_RANK], [NO_RANK] * 3]
            spec = Ranks(ranks, h, w, base)
            assert rank_items(ctx, items, bins, spec) == 0, last_error()
            want = expected(x, [b if b != NO_BIN else -1 for b in bins], ranks)
            same(spec, want, ("bins", h, w, base))
            assert (spec.get()[3] == JUNK).all() and (spec.get()[1, 1] == JUNK).all()
            assert spec.count.tolist() == (counts or [1, 2, 1, 0])
            again = Ranks(ranks, h, w, base)                         # a second run: the same bytes
            assert rank_items(ctx, items, bins, again) == 0
            assert again.get().tobytes() == spec.get().tobytes()
        assert items.untouched()
    # -0 counts as +0 and +0 is written (kernel_items plants -0 as bin 1's only value at pixel 0)
    assert want[0][1, 0, 0, 0] == 0


# ---- 2. every pass and every special value decides somewhere -------------------------------------------------------------------
def keys_of(x):
    with np.errstate(invalid="ignore"):
        u = (np.asarray(x, np.float32) + np.float32(0)).view(np.uint32)
    k = np.where(u >> 31 != 0, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k)


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def planted_items(h, w):
    """twelve items of N(5, 3) samples over a few decades with planted pixels in row 0, their values in shuffled item order"""
    r = np.random.default_rng(77)
    x = np.stack([(r.standard_normal((h, w)) * 3 + 5).astype(np.float32) * np.float32(10.0 ** (k % 4 - 1)) for k in range(12)])
    chain = [np.float32(1.0)]
    for _ in range(11):
        chain.append(np.nextafter(chain[-1], np.float32(2.0)))
    tiny = f32(np.arange(1, 13, dtype=np.uint32))                   # the twelve smallest positive denormals
    nans = [0x7FC00001, 0xFFC12345, 0x7F800001]                     # quiet, negative with a payload, signalling
    plant = [np.array(chain, np.float32),                                                    # only the last digit separates them
             np.array([3.5, -3.5] * 6, np.float32),                                          # differ only in sign
             np.full(12, 2.75, np.float32),                                                  # all equal
             np.array([0.0, -0.0] * 6, np.float32),                                          # the result must be +0
             np.array([-0.0] * 12, np.float32),
             np.array([np.inf, -np.inf, 1.0, -1.0] * 3, np.float32),
             np.full(12, -np.inf, np.float32),
             tiny, -tiny, np.concatenate([tiny[:6], -tiny[:5], [np.float32(0.0)]]).astype(np.float32),
             f32((nans + [0x3F800000, 0xC0000000, 0x40400000]) * 2),                         # NaN as some of the samples
             f32(nans * 4),                                                                  # NaN as all
             f32([0x7F800000] * 11 + [0xFFC12345])]
    for s in range(1, 8):                                            # twelve keys that agree above digit s and differ in it
        shift = 28 - 4 * s
        plant.append(f32([(0x41234567 & ~(0xF << shift) & 0xFFFFFFFF) | (d << shift) for d in range(12)]))
    perm = np.random.default_rng(5).permutation(12)
    for c, values in enumerate(plant):
        x[:, 0, c] = values[perm]
    return x, len(plant)


PLANTED_RANKS = [[0, 5, 6, 11]]


def test_every_pass_and_every_special_value_decides():
    h, w = 37, 53
    x, n_planted = planted_items(h, w)
    keys = keys_of(x).reshape(12, -1)
    order = np.sort(keys, axis=0)
    for s in range(8):                                               # the input's own precondition: pass s decides somewhere
        shift = 28 - 4 * s
        decided = 0
        for r in PLANTED_RANKS[0]:
            chosen = order[r]
            above = (keys.astype(np.uint64) >> (shift + 4)) == (chosen.astype(np.uint64) >> (shift + 4))[None]
            digit = (keys >> np.uint32(shift)) & np.uint32(15)
            for p in np.nonzero(above.sum(axis=0) > 1)[0][:4000]:
                if len(np.unique(digit[above[:, p], p])) > 1:
                    decided += 1
                    break
        assert decided, f"no pixel at which pass {s} decides"
    assert len(np.unique(order[:, 0] >> np.uint32(4))) == 1 and len(np.unique(order[:, 0])) == 12    # (the chain: the last digit alone)
    want = expected(x, None, PLANTED_RANKS)
    bits = want[0][0, :, 0, :n_planted]
    assert (bits[:, 3] == 0).all() and (bits[:, 4] == 0).all()                      # +0 for every zero
    assert (bits[:, 11] == NAN_BITS).all() and bits[3, 10] == NAN_BITS and bits[0, 10] != NAN_BITS and bits[3, 12] == NAN_BITS
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 1)
        spec = Ranks(PLANTED_RANKS, h, w)
        assert rank_items(ctx, items, None, spec) == 0, last_error()
        got = spec.get()
        for c in range(n_planted):
            assert got[0, :, 0, c].tobytes() == want[0][0, :, 0, c].tobytes(), f"planted pixel {c}"
        same(spec, want, "planted")
        assert items.untouched()


# ---- 3. alignment ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_alignment():
    x = R.kernel_items(37, 53)
    with L.Context(4, 64, 96) as ctx:
        seen = set()
        for item_base in range(4):
            for base in (0, 1):
                spec = Ranks(KERNEL_RANKS, 37, 53, base)
                assert rank_items(ctx, Guarded(x, item_base), KERNEL_BINS, spec) == 0, last_error()
                assert spec.out.sentinels_intact()
                seen.add(spec.get().tobytes())
        assert len(seen) == 1
        assert seen.pop() == expected(x, KERNEL_BINS, KERNEL_RANKS)[0].tobytes()


# ---- 4. refusals write nothing ----------------------------------------------------------------------------------------------------
def test_kernel_refusals_write_nothing():
    h, w = 37, 53
    x = R.kernel_items(h, w)
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 0)
        spec = Ranks(KERNEL_RANKS, h, w)
        before = spec.snapshot()

        def refused(bins=KERNEL_BINS, ptr=None, **fields):
            s = Ranks(KERNEL_RANKS, h, w)
            s.c.d_out, s.c.count = spec.c.d_out, spec.c.count
            for name, value in fields.items():
                setattr(s.c, name, value)
            b = None if bins is None else np.asarray(bins, np.uint32)
            rc = lib().ebcc_hip_rank_items(ctx.ptr, items.ptr if ptr is None else ptr[0], 5, None if b is None else b.ctypes.data, ctypes.byref(s.c))
            return rc == 1 and len(last_error()) > 0 and spec.snapshot() == before

        assert refused(bins=[0, 1, 4, 0, 2])                         # a bin >= n_bins
        assert refused(bins=[NO_BIN] * 5)                            # no item named
        assert refused(bins=[0, 1, 1, 1, 2])                         # rank 1 of bin 0, which now has one item
        assert refused(bins=[0, 1, 1, 0, 3])                         # bin 2 has a rank and no item; bin 3 an item and no rank: legal alone
        assert refused(rank=None) and refused(d_out=None) and refused(count=None)
        assert refused(n_bins=0) and refused(rows=0) and refused(cols=0)
        assert refused(n_ranks=0) and refused(n_ranks=17)
        assert refused(d_out=spec.c.d_out + 2)                       # d_out not 4-byte aligned
        assert refused(rows=2048) and refused(cols=2 ** 40, rows=2 ** 40)
        assert refused(ptr=[items.ptr + 2]) and refused(ptr=[None])  # items misaligned, items null
        all_unused = Ranks([[NO_RANK] * 3] * 4, h, w)
        all_unused.c.d_out, all_unused.c.count = spec.c.d_out, spec.c.count
        assert rank_items(ctx, items, KERNEL_BINS, all_unused) == 1 and last_error() and spec.snapshot() == before
        assert lib().ebcc_hip_rank_items(ctx.ptr, items.ptr, 5, None, None) == 1 and last_error()
        assert lib().ebcc_hip_rank_items(None, items.ptr, 5, None, ctypes.byref(spec.c)) == 1 and last_error()
        assert spec.snapshot() == before and items.untouched()
        assert rank_items(ctx, items, KERNEL_BINS, spec) == 0, last_error()               # and the context still works
        same(spec, expected(x, KERNEL_BINS, KERNEL_RANKS), "after refusals")


# ---- 5. launch limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equal", [False, True])
def test_past_a_launch_of_list_entries(equal):
    """70 000 items in one bin: past the 65 536 entries of a launch of k_rank_count (and past any 16-bit counter)"""
    n = 70000
    r = np.random.default_rng(11)
    x = np.stack([r.permutation(n) for _ in range(3)], axis=1).astype(np.float32).reshape(n, 1, 3)
    if equal:
        x[:, 0, 1] = np.float32(-7.5)
    ranks = [[0, 35000, 69999]]
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 1)
        spec = Ranks(ranks, 1, 3)
        assert rank_items(ctx, items, None, spec) == 0, last_error()
        got = spec.get().view(np.float32)
        for p in range(3):
            assert got[0, :, 0, p].tolist() == ([-7.5] * 3 if equal and p == 1 else [0.0, 35000.0, 69999.0]), p
        same(spec, expected(x, None, ranks), "70 000 items")
        assert spec.count.tolist() == [n] and items.untouched()


# ---- 6. streams against the oracle, across batches ----------------------------------------------------------------------------------
def series(h, w, n):
    """n frames of h x w at one scale, their streams from the product's encode (RELATIVE_ERROR 0.004, base_cr 20) and the oracle's
    decode of those streams; made once, never changed"""
    def make():
        L.oracle().orc_set_j2k_backend(0)
        x = np.stack([HB.inputs(h, w, [f])[0] for f in range(n)]).astype(np.float32)
        cfg = L.make_config((1, h, w), base_cr=20.0, error=0.004, residual_type=L.RELATIVE_ERROR)
        with L.Context(16, h, w) as ctx:
            streams = ctx.encode_frames(x, cfg)
        fields = np.stack([L.orc_decode(s).reshape(h, w) for s in streams])
        fields.setflags(write=False)
        return streams, fields
    return HB.once(("quantile series", h, w, n), make)


def largest_share(fields, bins, ranks):
    """over the used (bin, slot)s: the largest share of the pixels a single frame supplies"""
    table = np.asarray(ranks, np.uint64).reshape(len(ranks), -1)
    b = np.zeros(len(fields), np.int64) if bins is None else np.asarray(bins, np.int64)
    worst = 0.0
    for k in range(table.shape[0]):
        sel = fields[b == k]
        if len(sel):
            src = np.argsort(sel, axis=0, kind="stable")
            for r in table[k]:
                if int(r) != NO_RANK:
                    worst = max(worst, np.bincount(src[int(r)].ravel(), minlength=len(sel)).max() / src[0].size)
    return worst


def quantile(ctx, streams, bins, spec, row0=0, col0=0):
    keep, ptrs, sizes = R._args(streams)
    b = None if bins is None else np.asarray(bins, np.uint32)
    return lib().ebcc_hip_quantile_shard(ctx.ptr, ptrs, sizes, len(streams), None if b is None else b.ctypes.data, row0, col0, ctypes.byref(spec.c))


BINS12 = [f % 3 for f in range(12)]
ONE_RANKS = [[0, 3, 6, 11]]
BIN_RANKS = [[0, 3], [1, NO_RANK], [2, 1]]


def test_streams_against_the_oracle_across_batches(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)
    for bins, ranks, counts in ((None, ONE_RANKS, [12]), (BINS12, BIN_RANKS, [4, 4, 4])):
        assert largest_share(fields, bins, ranks) <= 0.5
        want = expected(fields, bins, ranks)
        seen = []
        for cap in (5, 16):                                          # three batches on two engine sets; one batch
            with L.Context(cap, H, W) as ctx:
                spec = Ranks(ranks, H, W, base=1)
                assert quantile(ctx, streams, bins, spec) == 0, last_error()
                same(spec, want, f"capacity {cap}, {len(ranks)} bins")
                seen.append(spec.get().tobytes())
                assert spec.count.tolist() == counts
        assert seen[0] == seen[1]


# ---- 7. a window -------------------------------------------------------------------------------------------------------------------
def test_window(monkeypatch):
    HB.use_env(monkeypatch, {})
    h, w, (row0, col0, rows, cols) = 90, 131, (9, 50, 40, 30)       # (crosses the code-block boundary at column 64)
    streams, fields = series(h, w, 6)
    ranks = [[0, 2, 5]]
    assert largest_share(fields, None, ranks) <= 0.5
    crop = fields[:, row0:row0 + rows, col0:col0 + cols]
    with L.Context(4, h, w) as ctx:                                 # (two batches)
        part = Ranks(ranks, rows, cols)
        assert quantile(ctx, streams, None, part, row0, col0) == 0, last_error()
        same(part, expected(crop, None, ranks), "window")
        whole = Ranks(ranks, h, w)                                   # the window that is the frame runs the whole-frame decode
        assert quantile(ctx, streams, None, whole) == 0, last_error()
        same(whole, expected(fields, None, ranks), "whole frame")
        assert part.get().tobytes() == np.ascontiguousarray(whole.get()[:, :, row0:row0 + rows, col0:col0 + cols]).tobytes()


# ---- 8. skipped frames -------------------------------------------------------------------------------------------------------------
def test_skipped_frames_are_not_read(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)
    bins, given = list(BINS12), list(streams)
    for f in (1, 4, 6, 11):
        bins[f], given[f] = NO_BIN, None
    kept = [f for f in range(12) if bins[f] != NO_BIN]
    ranks = [[0, 2], [1, NO_RANK], [2, 0]]                           # (bins of 3, 2 and 3 frames)
    with L.Context(5, H, W) as ctx:                                 # (eight named frames: two batches)
        spec = Ranks(ranks, H, W)
        assert quantile(ctx, given, bins, spec) == 0, last_error()
        same(spec, expected(fields[kept], [bins[f] for f in kept], ranks), "skipped")
        assert spec.count.tolist() == [3, 2, 3]
        idle = [[0, 2], [NO_RANK, NO_RANK], [2, 0]]                  # a bin whose slots are all unused: counted and not read
        both = [None if bins[f] in (1, NO_BIN) else streams[f] for f in range(12)]
        spec1 = Ranks(idle, H, W)
        assert quantile(ctx, both, bins, spec1) == 0, last_error()
        same(spec1, expected(fields[kept], [bins[f] for f in kept], idle), "a bin without a slot in use")
        assert spec1.count.tolist() == [3, 2, 3] and (spec1.get()[1] == JUNK).all()
        short = Ranks(ranks, H, W)                                   # the result is that of the shorter list
        assert quantile(ctx, [streams[f] for f in kept], [bins[f] for f in kept], short) == 0, last_error()
        assert short.get().tobytes() == spec.get().tobytes()


# ---- 9. special frames ---------------------------------------------------------------------------------------------------------------
def test_special_frames(monkeypatch):
    """a constant field, a frame without a residual layer and a legacy header-less stream in one list"""
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)

    def make():
        x = np.stack([np.full((H, W), 290.25, np.float32), HB.inputs(H, W, [20])[0]])
        with L.Context(4, H, W) as ctx:
            const = ctx.encode_frames(x[:1], L.make_config((1, H, W), base_cr=20.0, error=0.004, residual_type=L.RELATIVE_ERROR))[0]
            base_only = ctx.encode_frames(x[1:], L.make_config((1, H, W), base_cr=20.0, error=0.0, residual_type=L.NONE))[0]
        assert len(const) == 56
        return const, base_only
    const, base_only = HB.once("quantile special frames", make)
    mixed = [streams[0], const, L.legacy_repack(streams[1]), base_only, streams[2], streams[3]]
    decoded = np.stack([L.orc_decode(s).reshape(H, W) for s in mixed])
    assert np.array_equal(decoded[2], fields[1])
    ranks = [[0, 2, 3, 5]]
    with L.Context(4, H, W) as ctx:                                 # (two batches)
        spec = Ranks(ranks, H, W)
        assert quantile(ctx, mixed, None, spec) == 0, last_error()
        same(spec, expected(decoded, None, ranks), "special frames")


# ---- 10. refusals and a damaged stream ------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)
    with L.Context(5, 90, 131) as other:                            # a context of another geometry
        spec = Ranks(BIN_RANKS, H, W)
        before = spec.snapshot()
        assert quantile(other, streams, BINS12, spec) == 1 and last_error()
        assert spec.snapshot() == before
    with L.Context(5, H, W) as ctx:
        spec = Ranks(BIN_RANKS, H, W)
        before = spec.snapshot()
        bad = list(streams)
        bad[10] = bad[10][:40]                                      # a truncated header, in the last batch
        assert quantile(ctx, bad, BINS12, spec) == 1 and last_error()
        assert quantile(ctx, [None] + list(streams[1:]), BINS12, spec) == 1 and last_error()   # a named frame without a stream
        assert quantile(ctx, streams, BINS12, spec, row0=1) == 1 and last_error()              # the window leaves the frame
        assert quantile(ctx, streams, [0, 1, 3] * 4, spec) == 1 and last_error()               # a bin >= n_bins
        assert quantile(ctx, streams[:9], BINS12[:9], spec) == 1 and last_error()              # rank 3 of a bin of three frames
        assert spec.snapshot() == before
        assert quantile(ctx, streams, BINS12, spec) == 0, last_error()                         # and the context still works
        same(spec, expected(fields, BINS12, BIN_RANKS), "after refusals")


def test_a_stream_damaged_inside_a_batch(monkeypatch):
    """The damaged stream of tests/test_reduce_gpu.py::test_a_stream_damaged_inside_a_batch: its frame header parses, the decode of
    its batch refuses it - in the first pass.  The call returns 1 with d_out and count byte for byte what they were, and the next
    call on the context is correct."""
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)

    def make():
        with L.Context(4, H, W) as ctx:
            return ctx.encode_frames(L.era5_like(H, W, 64)[None], L.make_config((1, H, W), base_cr=10, residual_type=L.NONE))[0][:40]
    damaged = HB.once("quantile damaged stream", make)
    for cap, at in ((5, 8), (5, 1), (3, 4)):
        bad = list(streams)
        bad[at] = damaged
        with L.Context(cap, H, W) as ctx:
            spec = Ranks(BIN_RANKS, H, W, base=1)
            before = spec.snapshot()
            assert quantile(ctx, bad, BINS12, spec) == 1 and last_error()
            assert spec.snapshot() == before
            assert quantile(ctx, streams, BINS12, spec) == 0, last_error()
            same(spec, expected(fields, BINS12, BIN_RANKS), f"after the damaged stream at {at} of batches of {cap}")


# ---- 11. a reused context -------------------------------------------------------------------------------------------------------------
def test_a_reused_context(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = series(H, W, 12)
    originals = np.stack([HB.inputs(H, W, [f])[0] for f in range(12)]).astype(np.float32)
    row0, col0, rows, cols = 8, 16, 24, 40
    small_ranks = [[1, 4]]
    small_bins = [0 if f % 2 else NO_BIN for f in range(12)]         # six frames, one bin: fewer bins and a smaller window
    kept = [f for f in range(12) if small_bins[f] != NO_BIN]
    small_want = expected(fields[kept][:, row0:row0 + rows, col0:col0 + cols], None, small_ranks)
    with L.Context(5, H, W) as ctx:
        first = Ranks(BIN_RANKS, H, W)
        assert quantile(ctx, streams, BINS12, first) == 0, last_error()
        same(first, expected(fields, BINS12, BIN_RANKS), "first call")
        st = R.Stats(3, H, W).init(ctx)
        assert R.reduce(ctx, streams, BINS12, st) == 0, last_error()
        R.same(st.get(), R.expected(fields, BINS12, 3), "reduce on the same context")
        keep, ptrs, sizes = R._args(streams)
        report = np.zeros(12, A.FRAME_ERROR)
        rx = A.Resident(originals, 0)
        assert A.lib().ebcc_hip_audit_shard(ctx.ptr, ptrs, sizes, 12, rx.ptr, None, report.ctypes.data) == 0, last_error()
        for f in range(12):
            assert report[f]["max_abs"] == HB.stats(originals[f], fields[f])[0], f
        last = Ranks(small_ranks, rows, cols)
        assert quantile(ctx, streams, small_bins, last, row0, col0) == 0, last_error()
        same(last, small_want, "last call")
    with L.Context(5, H, W) as fresh:
        alone = Ranks(small_ranks, rows, cols)
        assert quantile(fresh, streams, small_bins, alone, row0, col0) == 0, last_error()
        assert alone.get().tobytes() == last.get().tobytes()


# ---- 12. Python ------------------------------------------------------------------------------------------------------------------------
def formula(fields, q, method):
    """the stated rule on sorted fields, in float64 -> float32 [rows][cols]"""
    order = np.sort(np.asarray(fields, np.float32) + np.float32(0), axis=0)
    h = np.float64(q) * np.float64(len(order) - 1)
    fl, ce = int(np.floor(h)), int(np.ceil(h))
    if method == "lower":
        return order[fl]
    if method == "higher":
        return order[ce]
    if method == "nearest":
        return order[int(np.rint(h))]
    if fl == ce:
        return order[fl]
    lo, hi = order[fl].astype(np.float64), order[ce].astype(np.float64)
    return (lo + (hi - lo) * (h - np.floor(h))).astype(np.float32)


def test_python_quantiles(monkeypatch):
    HB.use_env(monkeypatch, {})
    from ebcc_amd import h5_batch
    streams, fields = series(H, W, 12)
    qs = [0.0, 0.05, 0.5, 0.9, 1.0]
    bins = np.array([0] * 7 + [1] * 5)                               # (odd bins: the median is a sample)
    with h5_batch.BatchCodec(H, W, max_frames=5) as codec:
        for method in ("linear", "lower", "higher", "nearest"):
            one = codec.quantiles(streams, qs, method=method)
            assert one.values.shape == (1, 5, H, W) and one.values.dtype == np.float32 and one.count.tolist() == [12]
            for i, q in enumerate(qs):
                assert one.values[0, i].tobytes() == formula(fields, q, method).tobytes(), (method, q)
            two = codec.quantiles(streams, qs, bins=bins, n_bins=3, method=method)
            assert two.count.tolist() == [7, 5, 0] and np.isnan(two.values[2]).all()
            for k in range(2):
                for i, q in enumerate(qs):
                    assert two.values[k, i].tobytes() == formula(fields[bins == k], q, method).tobytes(), (method, k, q)
                assert two.values[k, 2].tobytes() == np.median(fields[bins == k].astype(np.float64), axis=0).astype(np.float32).tobytes()
        part = codec.quantiles(streams, 0.5, window=(9, 50, 40, 30))
        assert part.values.tobytes() == formula(fields[:, 9:49, 50:80], 0.5, "linear")[None, None].tobytes()
        with pytest.raises(ValueError, match="18"):
            codec.quantiles(streams * 3, [(2 * i + 0.5) / 35 for i in range(9)])              # (36 frames, h = 2 i + 0.5: ranks 0 .. 17)
        for bad in (dict(q=[1.5]), dict(q=[-0.1]), dict(q=[0.5], method="midpoint"), dict(q=[0.5], bins=[-1] * 12), dict(q=[0.5], bins=[0] * 11 + [1])):
            with pytest.raises(ValueError):
                codec.quantiles(streams, **bad)


def test_quantile_frames_of_a_dataset(tmp_path):
    """h5_batch.quantile_frames under an interpreter with h5py, as tests/test_reduce_gpu.py drives reduce_frames"""
    if not os.path.exists(T.CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([T.CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([T.CONDA_PY, os.path.join(L.ROOT, "tests", "h5_quantile.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 4, r.stdout
