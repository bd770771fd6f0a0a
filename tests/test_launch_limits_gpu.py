"""GPU: every count-limited launch loop of the host code driven past its limit - gridDim.y = 65535 (groups, chunks, boxes), 4096
frames a round of k_frame_errors, 65536 list entries a launch of k_time_fold, pieces of 2^20 floats of host_range_keys, and
frames * pieces > 65535 in one engine (from 8192 frames on the fused coarse levels are given up and `pieces` shrinks).

Every expected value is numpy's or the oracle's.  Expensive expectations are tiled over the entries, and the tiling never lines
up with a limit: each case first asserts, on its own expected data and without a device (the *_case functions), that the entry
at limit + k differs from the entries at k and at 0 for the first 64 k - a second launch that rereads the first launch's entries
cannot pass - and that the input has the property the test relies on.  Everything is compared by bytes, except the two sums of
the audit, which keep the bound tests/test_audit_gpu.py derives (through its `check`)."""
import ctypes

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L
from tests import test_audit_gpu as A
from tests import test_box_decode_gpu as B
from tests import test_container_encode_gpu as CE
from tests import test_group_encode_gpu as G
from tests import test_reduce_gpu as R
from tests import test_slab_decode_gpu as S
from tests import test_window_gpu as T

pytestmark = pytest.mark.gpu

GRID_Y = 65535                                        # gridDim.y: groups, chunks, boxes a launch; frames times pieces in an engine
ROUND_FRAMES = 4096                                   # frames a round of frame_errors
LIST_ENTRIES = 65536                                  # entries a launch of time_fold
HOST_PIECE = 1 << 20                                  # floats a piece of host_range_keys
SPARE = 64                                            # entries past a limit that must differ from those they would be mistaken for
EXACT = ("max_abs", "at", "n_over", "x_min", "x_max")


def past_the_limit(entry, limit, n):
    """entry(k) -> bytes: the entries at limit + k, for the first SPARE k that exist, differ from those at k and at 0"""
    first = entry(0)
    for k in range(min(SPARE, n - limit)):
        e = entry(limit + k)
        assert e != entry(k) and e != first, (limit, k)
    return n > limit


def error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


# ---- 1. ebcc_hip_frame_errors past 4096 frames ---------------------------------------------------------------------------------
def errors_case(n, h, w):
    """n frames of h x w and what was decoded of them, every value a small multiple of 2^-13 (all differences are exact in
    float).  Frame f: background errors of k / 16, k < 8; its largest error 1 + f / 8192 at pixel f % n_pix and once more at a
    later pixel (none behind the frame's last pixel); its own bound ((f % 7) + 1) / 16; its own minimum -(100 + f / 8) and
    maximum 200 + f / 4 at two further pixels.  -> (x, d, bound, numpy's report)"""
    n_pix = h * w
    f, i = np.arange(n, dtype=np.int32)[:, None], np.arange(n_pix, dtype=np.int32)[None, :]
    d = ((f * 7 + i * 3) % 32).astype(np.float32)
    x = d + ((i * 5 + f) % 8).astype(np.float32) / np.float32(16) * np.where((i + f) % 2, np.float32(-1), np.float32(1))
    f = np.arange(n)
    p = f % n_pix
    m = (1 + f / 8192).astype(np.float32)
    assert np.array_equal(m.astype(np.float64), 1 + f / 8192)
    p2 = p + 1 + f % 3
    later = p2 < n_pix
    x[f, p] = d[f, p] + m
    x[f[later], p2[later]] = d[f[later], p2[later]] + m[later]
    for at, value in (((p + 7) % n_pix, -(100 + f / 8)), ((p + 11) % n_pix, 200 + f / 4)):
        x[f, at] = d[f, at] = value.astype(np.float32)
    bound = (((f % 7) + 1) / 16).astype(np.float32)
    want = A.numpy_report(x.reshape(n, h, w), d.reshape(n, h, w), bound)
    assert np.array_equal(want["at"], p) and np.array_equal(want["max_abs"], m) and later[:SPARE].sum() > SPARE // 2
    assert np.array_equal(want["x_min"], -(100 + f / 8)) and np.array_equal(want["x_max"], 200 + f / 4)
    assert len(set(want["n_over"][:28].tolist())) > 3 and (want["n_over"] > 0).all()
    past_the_limit(lambda k: want[k].tobytes() + x[k].tobytes() + d[k].tobytes(), ROUND_FRAMES, n)
    return x.reshape(n, h, w), d.reshape(n, h, w), bound, want


@pytest.mark.parametrize("h,w,n", [(3, 5, ROUND_FRAMES), (3, 5, ROUND_FRAMES + 1), (3, 5, 2 * ROUND_FRAMES + 37), (90, 131, ROUND_FRAMES + 1)])
def test_frame_errors_past_a_round(h, w, n):
    """3 x 5: three quads and a tail of 3, one piece a frame; 90 x 131: two pieces a frame.  One round exactly, one frame into
    the second round, 37 frames into the third."""
    x, d, bound, want = errors_case(n, h, w)
    assert (h * w // 4, h * w % 4) == ((3, 3) if h == 3 else (2947, 2)) and max(1, h * w // 4096) == (1 if h == 3 else 2)
    call = A.lib().ebcc_hip_frame_errors
    with L.Context(4, 64, 96) as ctx:                                # (any context of the device)
        rx, rd = A.Resident(x, 1), A.Resident(d, 0)
        got = np.zeros(n, A.FRAME_ERROR)
        assert call(ctx.ptr, rx.ptr, rd.ptr, n, h, w, bound.ctypes.data, got.ctypes.data) == 0, error()
        A.check(got, want, x, d, f"{n} frames of {h}x{w}")
        # without bounds nothing is counted; the rest is the same
        free = np.zeros(n, A.FRAME_ERROR)
        assert call(ctx.ptr, rx.ptr, rd.ptr, n, h, w, None, free.ctypes.data) == 0, error()
        assert (free["n_over"] == 0).all()
        free["n_over"] = got["n_over"]
        assert free.tobytes() == got.tobytes()
        assert rx.untouched() and rd.untouched()
        if n > 2 * ROUND_FRAMES:                                     # a NaN in a frame of the third round
            bad = 2 * ROUND_FRAMES + 20
            nan = x.copy()
            nan[bad, 1, 2] = np.nan
            rn = A.Resident(nan, 3)
            again = np.zeros(n, A.FRAME_ERROR)
            assert call(ctx.ptr, rn.ptr, rd.ptr, n, h, w, bound.ctypes.data, again.ctypes.data) == 2
            others = np.arange(n) != bad
            for name in EXACT:
                assert again[name][others].tobytes() == want[name][others].tobytes(), name
            assert rn.untouched() and rd.untouched()


# ---- 2. ebcc_hip_time_fold past 65536 named items --------------------------------------------------------------------------------
FOLD_PATTERN = (0, 0, 0, 1, 1, 2, R.NO_BIN)            # item k names FOLD_PATTERN[k % 7]; bin 3 of 4 is never named
FOLD_ITEMS, FOLD_CUT, FOLD_ONE_BIN = 80000, 30011, 70000


def fold_case():
    """80 000 items of 1 x 7 (one quad and a tail of 3) with the scales of test_reduce_gpu.scale_of, their bins, and the expected
    bytes of: the four bins, the first 70 000 items in one bin"""
    def make():
        r = np.random.default_rng(80000)
        scale = np.array([R.scale_of(k) for k in range(FOLD_ITEMS)], np.float32)
        x = ((r.standard_normal((FOLD_ITEMS, 1, 7)) * 3 + 5).astype(np.float32) * scale[:, None, None]).astype(np.float32)
        bins = np.array([FOLD_PATTERN[k % 7] for k in range(FOLD_ITEMS)], np.uint32)
        x.setflags(write=False)
        bins.setflags(write=False)
        return x, bins, R.expected(x, bins, 4), R.expected(x[:FOLD_ONE_BIN], None, 1)
    x, bins, want, want_one = HB.once("launch limits: fold", make)
    named = np.flatnonzero(bins != R.NO_BIN)
    assert len(named) == 68572 and np.frombuffer(want["count"], np.uint64).tolist() == [34287, 22857, 11428, 0]
    order = named[np.argsort(bins[named], kind="stable")]           # the list as time_fold sorts it
    assert bins[order[LIST_ENTRIES]] == 2 and bins[order[LIST_ENTRIES - 1]] == 2 and bins[order[-1]] == 2       # the cut falls inside bin 2's run
    past_the_limit(lambda k: x[order[k]].tobytes(), LIST_ENTRIES, len(order))
    past_the_limit(lambda k: x[k].tobytes(), LIST_ENTRIES, FOLD_ONE_BIN)
    return x, bins, want, want_one


def test_the_order_of_the_long_folds_is_visible():
    """(no device) folding the same items in reverse order changes the bytes of both sums, in the four bins and in the one"""
    x, bins, _want, _one = fold_case()
    assert R.order_is_visible(x, bins, 4)
    assert R.order_is_visible(x[:FOLD_ONE_BIN], None, 1)


def fold_into(ctx, stats, items, first, n, bins):
    b = None if bins is None else np.ascontiguousarray(bins[first:first + n], np.uint32)
    return R.lib().ebcc_hip_time_fold(ctx.ptr, items.ptr + 4 * 7 * first, n, None if b is None else b.ctypes.data, ctypes.byref(stats.c))


def test_time_fold_past_a_launch():
    x, bins, want, want_one = fold_case()
    start = R.expected(x[:0], [], 4)                                # the initial values, which bin 3 keeps
    with L.Context(4, 64, 96) as ctx:                               # (any context of the device)
        items = R.Guarded(x, 1)
        st = R.Stats(4, 1, 7, base=1).init(ctx)
        assert fold_into(ctx, st, items, 0, FOLD_ITEMS, bins) == 0, error()
        got = st.get()
        R.same(got, want, "80 000 items, four bins")
        for name, _ in R.FIELDS:
            assert st.arrays[name].get()[3].tobytes() == np.frombuffer(start[name], st.arrays[name].dtype).reshape(st.shape)[3].tobytes(), name
        assert st.count.tolist() == [34287, 22857, 11428, 0]
        assert st.sentinels_intact() and items.untouched()
        # the same items in two calls
        two = R.Stats(4, 1, 7, base=1).init(ctx)
        assert fold_into(ctx, two, items, 0, FOLD_CUT, bins) == 0, error()
        assert fold_into(ctx, two, items, FOLD_CUT, FOLD_ITEMS - FOLD_CUT, bins) == 0, error()
        assert two.get() == got and two.sentinels_intact()
        # no list: one bin, whose accumulators are written back and loaded again across the cut
        one = R.Stats(1, 1, 7).init(ctx)
        assert fold_into(ctx, one, items, 0, FOLD_ONE_BIN, None) == 0, error()
        R.same(one.get(), want_one, "70 000 items, no list")
        assert one.count.tolist() == [FOLD_ONE_BIN] and one.sentinels_intact() and items.untouched()


# ---- 3. ebcc_hip_group_ranges past 65535 groups --------------------------------------------------------------------------------
RANGE_GROUPS = GRID_Y + 70
RANGE_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 63)
RANGE_NAN, RANGE_INF = GRID_Y + 3, 5


def ranges_case():
    """65 605 groups back to back in one buffer, one float of gap after every third.  Group g: minimum -(1 + g) / 2 at index
    g % n, maximum 1 + g / 4 at index (g + 1) % n (one float: the minimum alone); every 11th group has -0 as its maximum and
    every 13th -0 as its minimum.  -> (the buffer's words, offsets, lengths, the expected pairs [n][2] with -0 as +0)"""
    words, offsets, lengths = [np.full(R.FRONT, R.SENT, np.uint32)], [], []
    want = np.zeros((RANGE_GROUPS, 2), np.float32)
    at = R.FRONT
    for g in range(RANGE_GROUPS):
        n = RANGE_LENGTHS[g % 8]
        lo, hi = np.float32(-(1 + g) / 2), np.float32(1 + g / 4)
        x = np.full(n, 0.25, np.float32)
        if n == 1:
            x[0] = hi = lo
        elif g % 11 == 0:
            x[:] = -0.25
            x[g % n], x[(g + 1) % n], hi = lo, -0.0, np.float32(-0.0)
        elif g % 13 == 0:
            x[g % n], x[(g + 1) % n], lo = -0.0, hi, np.float32(-0.0)
        else:
            x[g % n], x[(g + 1) % n] = lo, hi
        assert x.min() == lo and x.max() == hi
        want[g] = (x.min() + np.float32(0), x.max() + np.float32(0))          # (-0 as +0)
        words.append(x.view(np.uint32))
        offsets.append(at)
        lengths.append(n)
        at += n
        if g % 3 == 2:
            words.append(np.full(1, R.SENT, np.uint32))
            at += 1
    words.append(np.full(R.BACK, R.SENT, np.uint32))
    offsets = np.array(offsets)
    assert float(-(1 + RANGE_GROUPS) / 2) == float(np.float32(-(1 + RANGE_GROUPS) / 2))
    assert all(set((offsets[np.array(lengths) == n] % 4).tolist()) == {0, 1, 2, 3} for n in RANGE_LENGTHS)      # every alignment of every length
    assert len({row.tobytes() for row in want}) == RANGE_GROUPS                # no two groups share a pair
    image = np.concatenate(words)
    minus_zero = [g for g in range(RANGE_GROUPS) if g != RANGE_NAN and (want[g] == 0).any()]
    assert all(np.signbit(image.view(np.float32)[offsets[g]:offsets[g] + lengths[g]]).any() for g in minus_zero)
    assert sum(g < GRID_Y for g in minus_zero) > 9000 and sum(g > GRID_Y for g in minus_zero) >= 8       # -0 as an extreme, in both launches
    assert (want.view(np.uint32) != 0x80000000).all()
    past_the_limit(lambda k: want[k].tobytes(), GRID_Y, RANGE_GROUPS)
    assert lengths[RANGE_NAN] == 3 and lengths[RANGE_INF] == 7
    return image, offsets, lengths, want


def test_group_ranges_past_a_launch():
    clean, offsets, lengths, want = ranges_case()
    planted = clean.copy()
    planted[offsets[RANGE_NAN] + 1] = np.array([np.nan], np.float32).view(np.uint32)[0]
    planted[offsets[RANGE_INF] + 6] = np.array([np.inf], np.float32).view(np.uint32)[0]
    marker = np.array([-123.0, -456.0], np.float32)
    with L.Context(2, 32, 48) as ctx:
        for image, bad in ((clean, ()), (planted, (RANGE_INF, RANGE_NAN))):
            d = L.DeviceArray(image)
            assert d.ptr % 256 == 0
            rc, mm, flags = G.group_ranges(ctx, [d.ptr + 4 * int(at) for at in offsets], lengths)
            assert rc == (2 if bad else 0), error()
            assert np.flatnonzero(flags).tolist() == list(bad) and set(flags.tolist()) <= {0, 1}
            expect = want.copy()
            for g in bad:
                expect[g] = marker                                   # (the pair of a group with a NaN or an Inf is not written)
            wrong = np.flatnonzero((mm.view(np.uint32) != expect.view(np.uint32)).any(axis=1))
            assert wrong.size == 0, (wrong[:8], mm[wrong[:8]], expect[wrong[:8]])
            assert np.array_equal(d.get(np.uint32, image.shape), image), "the input was written"
            d.free()


# ---- 4. ebcc_hip_gather_chunks past 65535 chunks -------------------------------------------------------------------------------
GATHER_DIMS, GATHER_CD = (1100, 40, 1000), (1, 32, 32)


def gather_case():
    """arbitrary 32-bit patterns (integer-valued floats cannot tell 44 M samples apart) and every padded chunk by clamped indexing"""
    def make():
        x = np.random.default_rng(1100).integers(0, 1 << 32, GATHER_DIMS, dtype=np.uint32).view(np.float32)
        want = CE.clamped_chunks(x, GATHER_CD, 0, 70400).view(np.uint32)
        x.setflags(write=False)
        want.setflags(write=False)
        return x, want
    x, want = HB.once("launch limits: gather", make)
    n = len(want)
    assert n == 1100 * 2 * 32 == 70400 and 40 - 32 == 8 and 1000 - 31 * 32 == 8
    c = np.arange(n)
    last_row, last_col = (c // 32) % 2 == 1, c % 32 == 31           # chunks with 8 real rows / 8 real columns
    for launch in (c < GRID_Y, c >= GRID_Y):                        # both launches hold edge chunks of both kinds
        assert (last_row & launch).any() and (last_col & launch).any() and (last_row & last_col & launch).any()
    assert last_row[GRID_Y + 33] and (want[GRID_Y + 33, 8:] == want[GRID_Y + 33, 7]).all() and (want[31, :, 8:] == want[31, :, 7:8]).all()      # (the padding repeats the edge)
    past_the_limit(lambda k: want[k].tobytes(), GRID_Y, n)
    return x, want


def test_gather_chunks_past_a_launch():
    x, want = gather_case()
    with L.Context(2, 32, 32) as ctx:
        src = CE.Resident(x, 1)
        for first, count, out_base in ((0, len(want), 0), (17, GRID_Y + 1, 3)):
            rc, got = CE.gather(ctx, src, GATHER_DIMS, GATHER_CD, first, count, out_base)
            assert rc == 0, error()
            expect = want[first:first + count].ravel()
            assert np.array_equal(got, expect), (first, count, np.flatnonzero(got != expect)[:4] // 1024, int((got != expect).sum()))
        assert src.unchanged()
        src.free()


# ---- 5. box and placed decode past 65535 boxes --------------------------------------------------------------------------------
BOX_H, BOX_W, BOX_CAPACITY = 64, 96, 2048
BOX_COUNTS = (30000, 30000, 6100, 200)                # boxes of frames 0 .. 3: the cut at 65535 falls inside frame 2's


def box_frames(monkeypatch):
    """four frames of 64 x 96 coded by the oracle - 0 and 2 with a residual layer, 1 and 3 constant - and the oracle's decode"""
    G.use_env(monkeypatch, "residual")

    def make():
        x = np.stack([L.era5_like(BOX_H, BOX_W, 5, 1.0, 0.6), np.full((BOX_H, BOX_W), 281.5, np.float32), L.era5_like(BOX_H, BOX_W, 6, 1.0, 0.6) + np.float32(100),
                      np.full((BOX_H, BOX_W), -3.25, np.float32)]).astype(np.float32)
        cfg = L.make_config((1, BOX_H, BOX_W), base_cr=20.0, error=0.02, residual_type=L.MAX_ERROR)
        streams, kinds = [], []
        for f in range(4):
            streams.append(L.orc_encode(x[f], cfg))
            kinds.append(L.trace()["residual"])
        assert kinds == ["trunc", "const", "trunc", "const"], kinds
        full = T.oracle_fields(streams, BOX_H, BOX_W)
        assert full[0].max() < full[2].min()                         # (no sample of frame 0 is one of frame 2)
        full.setflags(write=False)
        return streams, full
    return HB.once("launch limits: box frames", make)


def box_list(rows, cols):
    """66 300 boxes in frame order; the origin of box e walks over every position of the frame, so over every code-block"""
    e = np.arange(sum(BOX_COUNTS))
    frame = np.repeat(np.arange(4), BOX_COUNTS)
    boxes = np.stack([frame, (5 * e) % (BOX_H - rows + 1), (13 * e + e // 64) % (BOX_W - cols + 1)], axis=1)
    assert (np.diff(frame) >= 0).all() and frame[GRID_Y - 1] == frame[GRID_Y] == frame[GRID_Y + SPARE] == 2
    for f, least in ((0, 1.0), (2, 0.85)):                           # frame 0's boxes begin everywhere, frame 2's nearly
        seen = {(r, c) for _, r, c in boxes[frame == f].tolist()}
        assert len(seen) >= least * (BOX_H - rows + 1) * (BOX_W - cols + 1), (f, len(seen))
        assert {(r // 32, c // 32) for r, c in seen} == {(i, j) for i in range(2) for j in range(3)}
    return boxes


def box_crops(full, boxes, rows, cols):
    f, r0, c0 = boxes[:, 0, None, None], boxes[:, 1, None, None], boxes[:, 2, None, None]
    return full[f, r0 + np.arange(rows)[None, :, None], c0 + np.arange(cols)[None, None, :]]


@pytest.mark.parametrize("rows,cols", [(1, 1), (2, 3)], ids=["stations", "2x3"])
def test_boxes_past_a_launch(monkeypatch, rows, cols):
    streams, full = box_frames(monkeypatch)
    boxes = box_list(rows, cols)
    want = np.ascontiguousarray(box_crops(full, boxes, rows, cols)).view(np.uint32)
    assert np.array_equal(want[[0, 40000, GRID_Y + 5]], B.crops(full, boxes[[0, 40000, GRID_Y + 5]].tolist(), rows, cols).view(np.uint32))
    past_the_limit(lambda k: boxes[k].tobytes() + want[k].tobytes(), GRID_Y, len(boxes))
    with L.Context(BOX_CAPACITY, BOX_H, BOX_W) as ctx:              # (33 rounds of the context's capacity)
        got = B.boxes_of(ctx, streams, boxes, rows, cols).view(np.uint32)
        wrong = np.flatnonzero((got != want).any(axis=(1, 2)))
        assert wrong.size == 0, ("box list", len(wrong), wrong[:8], boxes[wrong[:8]].tolist())
        # the same list placed, a float of gap between the rectangles
        table, floats = S.laid_out([(f, r0, c0, rows, cols) for f, r0, c0 in boxes.tolist()], extra=0, gap=1)
        placed = S.expected(full, table, floats)
        assert (placed[rows * cols::rows * cols + 1] == S.SENT).all()
        for form, base in ((S.FORMS[0], 1),) + (((S.FORMS[2], 2),) if rows > 1 else ()):      # the host form once
            rc, out = S.raw_placed(ctx, streams, table, floats, form, base)
            assert rc == 0, (form, error())
            wrong = np.flatnonzero(out != placed)
            assert wrong.size == 0, (form, len(wrong), wrong[:8] // (rows * cols + 1))


class ChunksOfStreams:
    """what h5_batch.read_points uses of an h5py dataset of one-frame chunks: shape, id.read_direct_chunk"""

    def __init__(self, streams, h, w):
        self.streams, self.shape, self.id = streams, (len(streams), h, w), self

    def read_direct_chunk(self, offset):
        return 0, self.streams[offset[0]]


def test_read_points_past_a_launch(monkeypatch):
    from ebcc_amd import h5_batch
    streams, full = box_frames(monkeypatch)
    k = np.arange(16500)                                             # 66 000 boxes of 1 x 1: the cut falls among frame 3's
    r, c = (5 * k) % BOX_H, (13 * k + k // 64) % BOX_W
    want = full[:, r, c]
    assert 4 * len(k) > GRID_Y + SPARE and len(set(zip(r.tolist(), c.tolist()))) == BOX_H * BOX_W             # every pixel is a station
    with h5_batch.BatchCodec(BOX_H, BOX_W, max_frames=BOX_CAPACITY) as codec:
        got = h5_batch.read_points(ChunksOfStreams(streams, BOX_H, BOX_W), r, c, codec=codec)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ---- 6. one group larger than 2^20 floats in the host-groups form -------------------------------------------------------------
GROUP_FRAMES, GROUP_LOW, GROUP_HIGH = 180, 3, 177     # group A; the frames that hold its minimum and its maximum


def groups_case(monkeypatch):
    """Group A: 180 frames of 64 x 96 (1 105 920 floats: two pieces), six fields in rotation, RELATIVE_ERROR 0.002 of the group's
    range, whose minimum lies in frame 3 (first piece) and whose maximum in frame 177 (second piece).  Group B: three frames,
    MAX_ERROR 0.02.  -> (A, B, the oracle's 183 streams)"""
    G.use_env(monkeypatch, "residual")
    h, w = BOX_H, BOX_W

    def make():
        fields = np.stack([L.era5_like(h, w, 30 + i, 1.0 + 0.1 * (i % 4), 0.6) for i in range(6)]).astype(np.float32)
        low, high = fields[GROUP_LOW % 6].copy(), fields[GROUP_HIGH % 6].copy()
        low[11, 17], high[50, 70] = fields.min() - np.float32(40), fields.max() + np.float32(200)
        a = fields[np.arange(GROUP_FRAMES) % 6].copy()
        a[GROUP_LOW], a[GROUP_HIGH] = low, high
        b = np.stack([L.era5_like(h, w, 40 + i) for i in range(3)]).astype(np.float32)
        assert a.size > HOST_PIECE and (GROUP_LOW + 1) * h * w <= HOST_PIECE <= GROUP_HIGH * h * w
        assert np.argmin(a) // (h * w) == GROUP_LOW and np.argmax(a) // (h * w) == GROUP_HIGH
        flat = a.ravel()
        whole, first = float(flat.max() - flat.min()), float(flat[:HOST_PIECE].max() - flat[:HOST_PIECE].min())
        assert first < 0.5 * whole and flat[HOST_PIECE:].min() > flat.min()       # either piece alone gives another range

        def compat(frames):
            cfg = L.make_config((len(frames), h, w), (1, h, w), base_cr=15.0, error=0.002, residual_type=L.RELATIVE_ERROR)
            return G.entries(L.orc_encode(frames, cfg, "orc_ebcc_encode_chunking_compat"))
        distinct = compat(np.concatenate([fields, low[None], high[None]]))         # (the range of these eight is the group's)
        first_piece = compat(np.concatenate([fields, low[None]]))                  # the bound the first piece alone would give
        assert len(distinct) == 8 and all(distinct) and G.kinds(distinct).count("r") >= 6, G.kinds(distinct)
        assert all(distinct[k] != first_piece[k] for k in range(7))
        want = [distinct[6] if f == GROUP_LOW else distinct[7] if f == GROUP_HIGH else distinct[f % 6] for f in range(GROUP_FRAMES)]
        want += [L.orc_encode(b[f], L.make_config((1, h, w), base_cr=20.0, error=0.02, residual_type=L.MAX_ERROR)) for f in range(3)]
        assert all(want)
        return a, b, want
    return HB.once("launch limits: groups", make)


def test_host_group_larger_than_a_piece(monkeypatch):
    a, b, want = groups_case(monkeypatch)
    h, w = BOX_H, BOX_W
    keep_a, keep_b = a.copy(), b.copy()
    items = [(a.ctypes.data, GROUP_FRAMES, L.make_config((1, h, w), base_cr=15.0, error=0.002, residual_type=L.RELATIVE_ERROR), 1),
             (b.ctypes.data, 3, L.make_config((1, h, w), base_cr=20.0, error=0.02, residual_type=L.MAX_ERROR), 0)]
    with L.Context(64, h, w) as ctx:                                # (three batches)
        rc, got = G.encode_groups("host_frames", ctx, items, prefill=0xDEAD)
        assert rc == 0, error()
    wrong = [f for f in range(len(want)) if got[f] != want[f]]
    assert not wrong, (wrong[:8], [(len(got[f]), len(want[f])) for f in wrong[:8]])
    assert a.tobytes() == keep_a.tobytes() and b.tobytes() == keep_b.tobytes()


# ---- 7. 8192 frames and more in one engine ---------------------------------------------------------------------------------------
MANY_H, MANY_W, MANY, MANY_LIMIT = 256, 32, 8200, 8192      # 8 pieces a frame in both layers: frames * 8 > 65535 from 8192 frames on
MANY_WINDOW = (101, 7, 40, 20)
MANY_ERROR = 0.05


def field_of(f):
    """the field frame f holds: (f * 5) % 16 below 8192 frames; the frames from 8192 on are shifted by three fields, so that frame
    8192 + k holds neither frame k's field nor frame 0's"""
    return (f * 5 + 3 * (f // MANY_LIMIT)) % 16


def many_case(monkeypatch):
    """16 fields of 256 x 32 - era5_like at fourteen seeds, full-range noise, a constant -, the oracle's stream and decode of each"""
    G.use_env(monkeypatch, "residual")

    def make():
        fields = [L.era5_like(MANY_H, MANY_W, 50 + s, 1.0 + 0.1 * (s % 4), 0.6 + 0.3 * (s % 3)) for s in range(14)]
        fields.append(np.random.default_rng(7).uniform(-1000, 1000, (MANY_H, MANY_W)).astype(np.float32))
        fields.append(np.full((MANY_H, MANY_W), 12.5, np.float32))
        fields = np.stack(fields).astype(np.float32)
        cfg = L.make_config((1, MANY_H, MANY_W), base_cr=20.0, error=MANY_ERROR, residual_type=L.MAX_ERROR)
        streams, traces = [], []
        for x in fields:
            streams.append(L.orc_encode(x, cfg))
            traces.append(L.trace())
        assert all(streams) and len(set(streams)) == 16
        searched = [t["residual"] == "trunc" and t["trunc_steps"] > 0 for t in traces]
        assert sum(searched) >= 12 and traces[15]["residual"] == "const", [(t["residual"], t["trunc_steps"]) for t in traces]
        decoded = T.oracle_fields(streams, MANY_H, MANY_W)
        for a in (fields, decoded):
            a.setflags(write=False)
        return fields, streams, decoded
    fields, streams, decoded = HB.once("launch limits: many frames", make)
    which = np.array([field_of(f) for f in range(MANY)])
    assert np.array_equal(which[:MANY_LIMIT], (np.arange(MANY_LIMIT) * 5) % 16) and set(which[:16].tolist()) == set(range(16))
    past_the_limit(lambda k: streams[which[k]], MANY_LIMIT, MANY)
    rb_rows, top_rows = MANY_H + (-MANY_H) % 16, MANY_H                # the residual layer's padded grid; the top level's positions
    assert min(8, (rb_rows // 2) // 16) == 8 and min(8, top_rows // 16) == 8 and (MANY_LIMIT - 1) * 8 <= GRID_Y < MANY_LIMIT * 8
    return fields, streams, decoded, which


def many_frames_run(n_ctx, n, case):
    """encode, decode, window and audit of the first n frames on a context of n_ctx frames, each against the oracle"""
    fields, streams, decoded, which = case
    which = which[:n]
    x = fields[which]
    cfg = L.make_config((1, MANY_H, MANY_W), base_cr=20.0, error=MANY_ERROR, residual_type=L.MAX_ERROR)
    want = [streams[k] for k in which]
    with L.Context(n_ctx, MANY_H, MANY_W) as ctx:
        got = ctx.encode_frames(x, cfg)
        wrong = [f for f in range(n) if got[f] != want[f]]
        assert not wrong, ("encode", len(wrong), wrong[:8], [int(which[f]) for f in wrong[:8]])
        full = ctx.decode_frames(want)
        wrong = np.flatnonzero((full.view(np.uint32) != decoded[which].view(np.uint32)).any(axis=(1, 2)))
        assert wrong.size == 0, ("decode", len(wrong), wrong[:8], which[wrong[:8]])
        del full
        if n_ctx < MANY:
            return
        r0, c0, rows, cols = MANY_WINDOW
        win = T.window(ctx, want, MANY_WINDOW)
        crop = np.ascontiguousarray(decoded[which][:, r0:r0 + rows, c0:c0 + cols])
        wrong = np.flatnonzero((win.view(np.uint32) != crop.view(np.uint32)).any(axis=(1, 2)))
        assert wrong.size == 0, ("window", len(wrong), wrong[:8], which[wrong[:8]])
        # the audit of the streams against the originals: numpy on the oracle's decode
        bound = np.full(n, MANY_ERROR, np.float32)
        bound[1::2] = np.float32(MANY_ERROR / 4)                              # (n_over of a field then differs from frame to frame)
        per_field = {(k, b): HB.stats(fields[k], decoded[k], b) for k in range(16) for b in (bound[0], bound[1])}
        report = np.zeros(n, A.FRAME_ERROR)
        for f in range(n):
            report[f] = per_field[(which[f], bound[f])]
        keep, ptrs, sizes = T._args(want)
        rx = A.Resident(x, 1)
        audit = np.zeros(n, A.FRAME_ERROR)
        assert A.lib().ebcc_hip_audit_frames(ctx.ptr, ptrs, sizes, n, rx.ptr, bound.ctypes.data, audit.ctypes.data) == 0, error()
        A.check(audit, report, x, decoded[which], f"audit of {n} frames")
        assert rx.untouched()


def test_many_frames_in_one_engine(monkeypatch):
    """8200 frames in one engine of 8200 (past the limit: fused coarse levels given up, seven pieces), and the first 8191 in one of
    8191 (the last count below it): both held to the oracle, not to each other"""
    monkeypatch.setenv("EBCC_HIP_SLICES", "1")
    monkeypatch.delenv("EBCC_HIP_DECODE_SLICES", raising=False)
    case = many_case(monkeypatch)
    many_frames_run(MANY, MANY, case)
    many_frames_run(MANY_LIMIT - 1, MANY_LIMIT - 1, case)


# ---- 8. more than 65535 frames in one engine -------------------------------------------------------------------------------------
def test_a_context_past_the_grid_is_refused():
    lib = L.product()
    assert lib.ebcc_hip_create(0, GRID_Y + 1, 32, 32) is None
    assert "65535" in error() and "65536" in error(), error()
    L.oracle().orc_set_j2k_backend(0)
    x = L.kat_image(32, 32)
    cfg = L.make_config((1, 32, 32), base_cr=5.0, error=0.0, residual_type=L.NONE)
    with L.Context(4, 32, 32) as ctx:                               # a context made right after the refusal works
        assert ctx.encode_frames(x[None], cfg) == [L.orc_encode(x, cfg)]
