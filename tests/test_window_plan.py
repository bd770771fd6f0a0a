"""CPU tests of the window decode's dependency plan (ebcc_hip_window_plan, include/ebcc_hip.h): which code-blocks of a frame
a decode of a box needs.  The plan is held between two things this file works out on its own: it is SUFFICIENT - a float64
model of five inverse 9/7 levels gives the same box, exactly, with every dropped code-block zeroed - and it is no larger than
the plain radius-4 cone.  The library loads without a device (as test_boundary.py relies on); a missing symbol fails."""
import ctypes

import numpy as np
import pytest

from tests import _lib as L

GEOMETRIES = [(721, 1440), (257, 383), (64, 96), (100, 130), (2047, 33), (32, 2047)]
LEVELS = 5
N_RANDOM = 200


def _plan_fn():
    fn = L.product().ebcc_hip_window_plan              # AttributeError where the feature is missing: a failure, not a skip
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_size_t] * 6 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return fn


def plan(h, w, row0, col0, rows, cols):
    fn = _plan_fn()
    bands = np.full((16, 4), -7, np.int32)
    n = fn(h, w, row0, col0, rows, cols, bands.ctypes.data, None, 0)
    if n < 0:
        return n, None, None
    blocks = np.full((n, 6), -7, np.int32)
    assert fn(h, w, row0, col0, rows, cols, bands.ctypes.data, blocks.ctypes.data, n) == n
    return n, bands, blocks


# ---- the test's own geometry: sub-band sizes by ceiling division, code-blocks of 64 x 64 anchored at the origin -------------
def cdiv(a, b):
    return -(-a // b)


def res_size(n, r):
    """samples along one axis at resolution r (0 = the LL band, 5 = the frame)"""
    return cdiv(n, 1 << (LEVELS - r))


def band_shapes(h, w):
    """(height, width) of the 16 sub-bands: LL, then HL, LH, HH of the resolutions 1 .. 5"""
    out = [(res_size(h, 0), res_size(w, 0))]
    for r in range(1, LEVELS + 1):
        nh, nw = res_size(h, r), res_size(w, r)
        sh, sw = cdiv(nh, 2), cdiv(nw, 2)
        out += [(sh, nw - sw), (nh - sh, sw), (nh - sh, nw - sw)]
    return out


def block_list(h, w):
    """[band, x0, x1, y0, y1] of every code-block: band by band, rows of code-blocks top to bottom"""
    out = []
    for b, (bh, bw) in enumerate(band_shapes(h, w)):
        for cy in range(cdiv(bh, 64)):
            for cx in range(cdiv(bw, 64)):
                out.append([b, cx * 64, min(bw, cx * 64 + 64), cy * 64, min(bh, cy * 64 + 64)])
    return np.array(out, np.int32)


# ---- the test's own inverse 9/7: lifting with whole-sample symmetric extension, float64 -------------------------------------
ALPHA, BETA, GAMMA, DELTA, KAPPA = -1.586134342059924, -0.052980118572961, 0.882911075530934, 0.443506852043971, 1.230174104914001


def inverse_axis(low, high, axis):
    """one inverse level along `axis`: low-pass and high-pass halves -> the interleaved samples"""
    low, high = np.moveaxis(low, axis, 0), np.moveaxis(high, axis, 0)
    n = low.shape[0] + high.shape[0]
    x = np.empty((n,) + low.shape[1:], np.float64)
    x[0::2] = low * KAPPA
    x[1::2] = high * (1.0 / KAPPA)
    if n > 1:
        ne, no = low.shape[0], high.shape[0]
        for parity, c in ((0, DELTA), (1, GAMMA), (0, BETA), (1, ALPHA)):
            xp = np.pad(x, [(1, 1)] + [(0, 0)] * (x.ndim - 1), mode="reflect")     # x[-1] = x[1], x[n] = x[n - 2]
            cnt = ne if parity == 0 else no
            left, right = xp[parity:n + parity:2][:cnt], xp[parity + 2::2][:cnt]
            x[parity::2] -= c * (left + right)
    return np.moveaxis(x, 0, axis)


def synthesise(bands):
    ll = bands[0]
    for r in range(1, LEVELS + 1):
        hl, lh, hh = bands[3 * r - 2], bands[3 * r - 1], bands[3 * r]
        lo = inverse_axis(ll, hl, 1)          # rows of the low-pass half
        hi = inverse_axis(lh, hh, 1)          # rows of the high-pass half
        ll = inverse_axis(lo, hi, 0)
    return ll


# ---- windows -----------------------------------------------------------------------------------------------------------------
def axis_edges(n):
    """positions on and one beside multiples of 64 * 2^k (the first and the last multiple inside the axis, for every k)"""
    e = set()
    for k in range(LEVELS + 1):
        m = 64 << k
        for j in {1, (n - 1) // m}:
            for d in (-1, 0, 1):
                if j >= 1 and 0 < j * m + d < n:
                    e.add(j * m + d)
    return sorted(e)


def catalogue(h, w, rng):
    wins = []
    ch, cw = min(h, 19), min(w, 23)
    for r0 in (0, h - ch):
        for c0 in (0, w - cw):
            wins += [(r0, c0, ch, cw), (r0 if r0 == 0 else h - 1, c0 if c0 == 0 else w - 1, 1, 1)]      # every corner, as a box and as 1 x 1
    wins += [(h // 2, w // 2, 1, 1), (h // 3, 2 * w // 3, 1, 1)]
    wins += [(h // 2, 0, 1, w), (0, 0, 1, w), (h - 1, 0, 1, w)]                                             # full rows
    wins += [(0, w // 2, h, 1), (0, 0, h, 1), (0, w - 1, h, 1)]                                             # full columns
    for e in axis_edges(h):                                                                                 # a box that starts / ends at the edge
        c0 = int(rng.integers(0, w)); cols = int(rng.integers(1, w - c0 + 1))
        top = max(0, e - int(rng.integers(1, 40)))
        wins += [(e, c0, min(h - e, int(rng.integers(1, 40))), cols), (top, c0, e - top, cols)]
    for e in axis_edges(w):
        r0 = int(rng.integers(0, h)); rows = int(rng.integers(1, h - r0 + 1))
        left = max(0, e - int(rng.integers(1, 40)))
        wins += [(r0, e, rows, min(w - e, int(rng.integers(1, 40)))), (r0, left, rows, e - left)]
    return wins


def random_windows(h, w, rng, n):
    wins = []
    for _ in range(n):
        r0, c0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        if rng.random() < 0.5:                                      # small boxes as often as arbitrary ones
            rows, cols = int(rng.integers(1, min(h - r0, 48) + 1)), int(rng.integers(1, min(w - c0, 48) + 1))
        else:
            rows, cols = int(rng.integers(1, h - r0 + 1)), int(rng.integers(1, w - c0 + 1))
        wins.append((r0, c0, rows, cols))
    return wins


def all_windows(h, w):
    rng = np.random.default_rng(h * 10007 + w)
    wins = catalogue(h, w, rng) + random_windows(h, w, rng, N_RANDOM)
    assert all(rows >= 1 and cols >= 1 and r0 + rows <= h and c0 + cols <= w for r0, c0, rows, cols in wins)
    return wins


def radius4_cone(h, w, win):
    """needed rectangle [x0, x1, y0, y1] of every sub-band by the plain rule: every output sample of a level depends on the
    interleaved positions within +-4"""
    r0, c0, rows, cols = win

    def axis(n, a, b):                       # outputs [a, b) of n samples -> low-pass range, high-pass range
        lo, hi = max(0, a - 4), min(n - 1, b - 1 + 4)
        return ((lo + 1) // 2, hi // 2 + 1), (lo // 2, (hi + 1) // 2)

    out = [None] * 16
    x, y = (c0, c0 + cols), (r0, r0 + rows)
    for r in range(LEVELS, 0, -1):
        (lx, hx), (ly, hy) = axis(res_size(w, r), *x), axis(res_size(h, r), *y)
        out[3 * r - 2], out[3 * r - 1], out[3 * r] = hx + ly, lx + hy, hx + hy
        x, y = lx, ly
    out[0] = x + y
    return out


def meets(rect, need):
    return need[0] < need[1] and need[2] < need[3] and rect[0] < need[1] and need[0] < rect[1] and rect[2] < need[3] and need[2] < rect[3]


# ---- 1. full window ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_full_window_keeps_everything(h, w):
    n, bands, blocks = plan(h, w, 0, 0, h, w)
    want = block_list(h, w)
    assert n == len(want)
    if (h, w) == (721, 1440):
        assert n == 298
    assert np.array_equal(blocks[:, :5], want)
    assert (blocks[:, 5] == 1).all()
    for b, (bh, bw) in enumerate(band_shapes(h, w)):
        if bh == 0 or bw == 0:
            assert bands[b][0] == bands[b][1] or bands[b][2] == bands[b][3]
        else:
            assert list(bands[b]) == [0, bw, 0, bh], (b, list(bands[b]))


# ---- 2. sufficiency and 3. tightness -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_plan_is_sufficient_and_inside_radius_4(h, w):
    shapes = band_shapes(h, w)
    want_blocks = block_list(h, w)
    wins = all_windows(h, w)
    assert len(wins) >= N_RANDOM + 20
    checked = 0
    for k, win in enumerate(wins):
        r0, c0, rows, cols = win
        n, bands, blocks = plan(h, w, r0, c0, rows, cols)
        assert n == len(want_blocks), win
        assert np.array_equal(blocks[:, :5], want_blocks), win
        # tightness: keep says what `bands` says, the needed rectangles lie inside the sub-band and inside the radius-4 cone
        cone = radius4_cone(h, w, win)
        for b, (bh, bw) in enumerate(shapes):
            x0, x1, y0, y1 = (int(v) for v in bands[b])
            assert 0 <= x0 <= x1 <= bw and 0 <= y0 <= y1 <= bh, (win, b)
            if x0 < x1 and y0 < y1:
                c = cone[b]
                assert c[0] <= x0 and x1 <= c[1] and c[2] <= y0 and y1 <= c[3], (win, b, list(bands[b]), c)
        for blk in blocks:
            b, rect, keep = int(blk[0]), [int(v) for v in blk[1:5]], int(blk[5])
            assert keep == (1 if meets(rect, [int(v) for v in bands[b]]) else 0), (win, list(blk))
            if keep:
                assert meets(rect, cone[b]), (win, list(blk))
        # sufficiency: zero every coefficient of every dropped code-block; the window of the synthesis does not change
        rng = np.random.default_rng(1000 * k + h + w)
        coeff = [rng.standard_normal(s) * 100.0 for s in shapes]
        masked = [c.copy() for c in coeff]
        for blk in blocks:
            if not blk[5]:
                masked[blk[0]][blk[3]:blk[4], blk[1]:blk[2]] = 0.0
        full = synthesise(coeff)
        assert full.shape == (h, w)
        part = synthesise(masked)
        a, b_ = full[r0:r0 + rows, c0:c0 + cols], part[r0:r0 + rows, c0:c0 + cols]
        assert np.array_equal(a, b_), (win, int((a != b_).sum()))
        checked += 1
    assert checked == len(wins)                                      # no window left out


def test_small_windows_drop_most_code_blocks():
    # (a plan that keeps everything would pass the checks above: a 32 x 32 box of a 721 x 1440 frame needs a small part)
    n, bands, blocks = plan(721, 1440, 300, 700, 32, 32)
    assert n == 298 and 0 < int(blocks[:, 5].sum()) <= 40


# ---- 4. invalid windows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(721, 1440), (64, 96)])
def test_invalid_windows(h, w):
    big = (1 << 64) - 1
    bad = [(0, 0, 0, w), (0, 0, h, 0), (0, 0, 0, 0),                                    # empty
           (h, 0, 1, 1), (0, w, 1, 1), (0, 0, h + 1, w), (0, 0, h, w + 1), (1, 0, h, w), (0, 1, h, w), (h - 1, w - 1, 2, 1), (h - 1, w - 1, 1, 2),
           (big, 0, 2, 1), (0, big, 1, 2), (1, 0, big, 1), (0, 1, 1, big), (big, big, big, big), (2, 0, big - 1, 1), (0, 2, 1, big - 1)]     # sums that wrap
    for win in bad:
        n, _, _ = plan(h, w, *win)
        assert n == -1, win
    assert plan(h, w, h - 1, w - 1, 1, 1)[0] > 0
    # ... and a geometry the engine refuses
    assert plan(0, 10, 0, 0, 1, 1)[0] == -1 and plan(2048, 10, 0, 0, 1, 1)[0] == -1
