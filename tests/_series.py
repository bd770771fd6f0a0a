"""The area series of include/ebcc_hip.h restated with numpy, and its C types for ctypes - shared by tests/test_series_check.py,
tests/test_series_gpu.py and tests/h5_series.py (numpy and ctypes alone: the child interpreter of the h5py test imports it).

The rule, as the header states it:

    fold64(v, g): 64 partial sums, +0.0 at first; partial l adds the elements i with (i / g) % 64 == l in increasing i; then
    p[l] = p[l] + p[l ^ o] for o = 32, 16, 8, 4, 2, 1; the result is p[0].
    per pixel  w = w_row[r] * (double) w_pix[r][c] (1 where an array is missing); w == 0: the pixel takes part in nothing;
               t_sum = (double) x * w, t_sq = ((double) x * (double) x) * w, t_over = x > threshold ? w : 0.0 (in float)
    per row    fold64 over the row's terms with g = 4, columns counted from the region's first column
    per region fold64 over the row results with g = 1
    min / max  in float, + 0.0f on the way out; no live pixel: +inf / -inf

Here the terms are padded with +0.0 - an identity, since a partial that starts at +0.0 never becomes -0.0 - to whole rounds of
64 groups and reshaped to [rounds][64][g]."""
import ctypes

import numpy as np

AREA_STAT = np.dtype([("sum", "<f8"), ("sum_sq", "<f8"), ("over", "<f8"), ("min", "<f4"), ("max", "<f4")])
assert AREA_STAT.itemsize == 32
FIELDS = ("sum", "sum_sq", "over", "min", "max")
_LANES = np.arange(64)


class Region(ctypes.Structure):
    """ebcc_hip_region"""
    _fields_ = [("row0", ctypes.c_size_t), ("col0", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t)]


class AreaSpec(ctypes.Structure):
    """ebcc_hip_area_spec"""
    _fields_ = [("n_regions", ctypes.c_size_t), ("regions", ctypes.c_void_p), ("w_row", ctypes.c_void_p), ("d_w_pix", ctypes.c_void_p),
                ("use_threshold", ctypes.c_int), ("threshold", ctypes.c_float)]


def region_array(regions):
    """(row0, col0, rows, cols) tuples as a ctypes array of ebcc_hip_region"""
    return (Region * len(regions))(*[Region(*(int(v) for v in r)) for r in regions])


def fold64(v, g):
    """fold64 over the last axis of the float64 array v"""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    rounds = max(1, -(-n // (64 * g)))
    t = np.zeros(v.shape[:-1] + (rounds * 64 * g,), np.float64)
    t[..., :n] = v
    t = t.reshape(v.shape[:-1] + (rounds, 64, g))
    p = np.zeros(v.shape[:-1] + (64,), np.float64)
    for k in range(rounds):
        for j in range(g):
            p = p + t[..., k, :, j]
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[..., _LANES ^ o]
    return p[..., 0]


def terms(x, region, w_row=None, w_pix=None, threshold=None):
    """(t_sum, t_sq, t_over, live, samples) of one region of the fields x [n][H][W] float32: the terms [n][rows][cols] in float64
    - +0.0 where the weight is 0 -, the live pixels [rows][cols] and the region's samples"""
    row0, col0, rows, cols = (int(v) for v in region)
    xs = np.asarray(x, np.float32)[:, row0:row0 + rows, col0:col0 + cols]
    wr = np.ones(rows, np.float64) if w_row is None else np.asarray(w_row, np.float64)[row0:row0 + rows]
    wp = np.ones((rows, cols), np.float64) if w_pix is None else np.asarray(w_pix, np.float32)[row0:row0 + rows, col0:col0 + cols].astype(np.float64)
    w = wr[:, None] * wp
    live = w != 0.0
    xd = xs.astype(np.float64)
    zero = np.float64(0.0)
    t_sum = np.where(live, xd * w, zero)
    t_sq = np.where(live, (xd * xd) * w, zero)
    over = np.zeros(xs.shape, bool) if threshold is None else xs > np.float32(threshold)
    t_over = np.where(live & over, np.broadcast_to(w, xs.shape), zero)
    return t_sum, t_sq, t_over, live, xs


def region_stats(x, region, w_row=None, w_pix=None, threshold=None):
    """the records [n] (AREA_STAT) of one region"""
    t_sum, t_sq, t_over, live, xs = terms(x, region, w_row, w_pix, threshold)
    out = np.zeros(len(xs), AREA_STAT)
    for name, t in (("sum", t_sum), ("sum_sq", t_sq), ("over", t_over)):
        out[name] = fold64(fold64(t, 4), 1)
    flat_live = np.broadcast_to(live, xs.shape).reshape(len(xs), -1)
    flat = xs.reshape(len(xs), -1)
    out["min"] = np.where(flat_live, flat, np.float32(np.inf)).min(axis=1) + np.float32(0.0)
    out["max"] = np.where(flat_live, flat, np.float32(-np.inf)).max(axis=1) + np.float32(0.0)
    return out


def expected(x, regions, w_row=None, w_pix=None, threshold=None):
    """the records [n][R] of a list of regions"""
    return np.stack([region_stats(x, r, w_row, w_pix, threshold) for r in regions], axis=1)


def left_to_right(x, region, w_row=None, w_pix=None):
    """the sum of the same terms by a plain loop, pixel after pixel in row-major order: [n] float64"""
    t_sum = terms(x, region, w_row, w_pix)[0]
    return np.cumsum(t_sum.reshape(len(t_sum), -1), axis=1)[:, -1]


def total_weight(regions, h, w, w_row=None, w_pix=None):
    """the weight of every region, order-free (math.fsum): [R] float64"""
    import math
    out = []
    for row0, col0, rows, cols in regions:
        wr = np.ones(rows, np.float64) if w_row is None else np.asarray(w_row, np.float64)[row0:row0 + rows]
        wp = np.ones((rows, cols), np.float64) if w_pix is None else np.asarray(w_pix, np.float32)[row0:row0 + rows, col0:col0 + cols].astype(np.float64)
        out.append(math.fsum((wr[:, None] * wp).ravel().tolist()))
    return np.array(out, np.float64)
