"""The regrid rule of include/ebcc_hip.h restated with numpy - shared by tests/test_regrid_check.py, tests/test_regrid_maps.py,
tests/test_regrid_gpu.py and tests/h5_regrid.py (numpy and ctypes alone: the child interpreter of the h5py test imports it).

The rule, as the header states it, for output (R, C) of a frame with float samples x:

    a = +0.0;  for i = 0 .. rows.count[R), increasing:  r = rows.first[R] + i
        t = +0.0;  for j = 0 .. cols.count[C), increasing:  t = t + (double) x[r][col(C, j)] * wc[C][j]
        a = a + wr[R][i] * t
    out[R][C] = (float) a;   col(C, j) = cols.first[C] + j, % width when the column map wraps

Here every support is padded to the longest of its axis with taps of weight +0.0 (on an index inside the axis) - an identity for
finite samples, since an accumulator that starts at +0.0 never becomes -0.0 - and the loops over the taps run over whole arrays,
with separate multiply and add.  It follows that a sample of -0 under a weight of 1 leaves as +0: the identity map returns the
bytes of x + 0.0f."""
import ctypes

import numpy as np

from ebcc_amd import regrid as M

AxisMapC, RegridSpec = M.AxisMapC, M.RegridSpec


class Region(ctypes.Structure):
    """ebcc_hip_region"""
    _fields_ = [("row0", ctypes.c_size_t), ("col0", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t)]


def padded(m, extent):
    """(index [n_out][L], weight [n_out][L]) of an AxisMap over an axis of `extent` positions: L the longest support"""
    L = int(m.count.max())
    j = np.arange(L)[None, :]
    idx = m.first.astype(np.int64)[:, None] + j
    idx = idx % extent if m.wrap else np.minimum(idx, extent - 1)
    w = np.zeros((m.n_out, L), np.float64)
    real = j < m.count.astype(np.int64)[:, None]
    w[real] = m.weight                                                  # (packed output by output: the row-major order of `real`)
    idx = np.where(real, idx, m.first.astype(np.int64)[:, None])
    return idx, w


def apply(x, row_map, col_map, acc=np.float64, reverse=False):
    """the rule on x [n][H][W] float32 -> [n][Ro][Co] float32.  acc: the type of products and sums (float64 is the rule);
    reverse: the taps in decreasing order - the two wrong readings the tests tell the rule from"""
    x = np.asarray(x, np.float32)
    n, H, W = x.shape
    ir, wr = padded(row_map, H)
    ic, wc = padded(col_map, W)
    wr, wc = wr.astype(acc), wc.astype(acc)
    xa = x.astype(acc)
    order = (lambda L: range(L - 1, -1, -1)) if reverse else range
    t = np.zeros((n, H, col_map.n_out), acc)
    for j in order(ic.shape[1]):
        p = xa[:, :, ic[:, j]] * wc[None, None, :, j]
        t = t + p
    a = np.zeros((n, row_map.n_out, col_map.n_out), acc)
    for i in order(ir.shape[1]):
        p = wr[None, :, i, None] * t[:, ir[:, i], :]
        a = a + p
    return a.astype(np.float32)


SCALES = (np.float32(1e-6), np.float32(1.0), np.float32(1e6))


def items(h, w, n=3):
    """n items of h x w.  Items 0, 2, ..: N(5, 3) samples, blocks of two rows and of two columns scaled by 1e-6, 1, 1e6 in turn,
    -0 planted (the inputs of tests/test_series_gpu.py).  The output is float32, and a float64 sum of such terms in another order
    differs by parts in 2^52 - the cast hides it.  Odd items therefore cancel: samples of scale 1e-6 everywhere, and pairs
    +V, -V of scale 1e6 two positions apart - along the columns (4m, 4m + 2) in the left half, along the rows in the right
    half.  A support that holds a pair sums to something of scale 1e-6 through partial sums of scale 1e6: which tiny samples
    are rounded against the large one depends on the order (in increasing order the sample behind the pair is added exactly,
    in decreasing order the one between them), and shows in the float32 result."""
    r = np.random.default_rng(h * 1000 + w)
    x = (r.standard_normal((n, h, w)) * 3 + 5).astype(np.float32)
    rows, cols = np.arange(h)[:, None], np.arange(w)[None, :]
    x = x * np.asarray(SCALES, np.float32)[(rows // 2 + cols // 2 + 1) % 3][None]
    x[0, 0, 0] = x[n - 1, h - 1, w - 1] = -0.0
    for k in range(1, n, 2):
        tiny = ((r.standard_normal((h, w)) * 3 + 5) * 1e-6).astype(np.float32)
        big = ((r.standard_normal((h, w)) * 3 + 5) * 1e6).astype(np.float32)
        half = w // 2
        for c in range(0, half - 2, 4):
            tiny[:, c], tiny[:, c + 2] = big[:, c], -big[:, c]
        for q in range(0, h - 2, 4):
            tiny[q, half:], tiny[q + 2, half:] = big[q, half:], -big[q, half:]
        x[k] = tiny
    return np.ascontiguousarray(x, np.float32)


def order_is_visible(x, row_map, col_map):
    """the rule's bytes differ from those of float32 accumulation and from those of the taps in reverse"""
    want = apply(x, row_map, col_map).tobytes()
    return want != apply(x, row_map, col_map, acc=np.float32).tobytes() and want != apply(x, row_map, col_map, reverse=True).tobytes()


def bounding(row_map, col_map, H, W):
    """(row0, col0, rows, cols) of what the map reads of an H x W frame: the whole width when a column support wraps"""
    def span(m, extent):
        f, c = m.first.astype(np.int64), m.count.astype(np.int64)
        if (f + c > extent).any():
            return 0, extent
        return int(f.min()), int((f + c).max())
    r0, r1 = span(row_map, H)
    c0, c1 = span(col_map, W)
    return r0, c0, r1 - r0, c1 - c0
