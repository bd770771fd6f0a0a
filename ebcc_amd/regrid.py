"""Maps of the regrid decode (include/ebcc_hip.h: ebcc_hip_axis_map, ebcc_hip_regrid_spec) - numpy and ctypes alone, no device.

A regrid is a separable linear map: along each axis every output position has a contiguous support of source positions
[first, first + count) and one float64 weight per tap.  AxisMap holds one axis in the packed form the C interface takes; the
builders make the usual ones.  Weights are used by the library as given - whatever normalisation a map wants is done here.

    rows = conservative_map(cell_edges(lat, -90, 90), cell_edges(lat_1deg, -90, 90), measure=lambda e: np.sin(np.deg2rad(e)))
    cols = conservative_map(cell_edges(lon), cell_edges(lon_1deg), period=360.0)
    coarse = codec.regrid(streams, rows, cols)                        # (n, 181, 360) float32, h5_batch.BatchCodec
"""
import ctypes
import math

import numpy as np

MAX_TAPS = 256                                        # EBCC_HIP_REGRID_MAX_TAPS
MAX_OUT = 65535


class AxisMapC(ctypes.Structure):
    """ebcc_hip_axis_map"""
    _fields_ = [("n_out", ctypes.c_size_t), ("first", ctypes.c_void_p), ("count", ctypes.c_void_p), ("weight", ctypes.c_void_p),
                ("wrap", ctypes.c_int)]


class RegridSpec(ctypes.Structure):
    """ebcc_hip_regrid_spec"""
    _fields_ = [("rows", AxisMapC), ("cols", AxisMapC)]


class AxisMap:
    """One axis of a regrid: first (n_out,) and count (n_out,) as uint32, weight the packed float64 weights - those of output 0,
    then of output 1, ... -, wrap: tap j of output i reads source index (first[i] + j) % extent (columns only).  ValueError for
    what no extent could make valid; whether the supports fit a frame is the library's check (ebcc_hip_regrid_check)."""

    def __init__(self, first, count, weight, wrap=False):
        f, c = np.asarray(first), np.asarray(count)
        if f.ndim != 1 or c.shape != f.shape or f.size < 1 or f.size > MAX_OUT or f.dtype.kind not in "iu" or c.dtype.kind not in "iu":
            raise ValueError(f"first and count must be integer arrays of one length, 1 .. {MAX_OUT}")
        if f.min() < 0 or f.max() >= 2 ** 32 or c.min() < 1 or c.max() > MAX_TAPS:
            raise ValueError(f"first must not be negative and count must lie in 1 .. {MAX_TAPS}")
        self.first, self.count = np.ascontiguousarray(f, np.uint32), np.ascontiguousarray(c, np.uint32)
        self.weight = np.ascontiguousarray(weight, np.float64)
        if self.weight.shape != (int(self.count.sum()),):
            raise ValueError(f"weight must hold the {int(self.count.sum())} weights of the supports, packed")
        if not np.isfinite(self.weight).all():
            raise ValueError("a weight is a NaN or an Inf")
        self.wrap = bool(wrap)

    @property
    def n_out(self):
        return self.first.size

    @property
    def offsets(self):
        """where the weights of every output begin in `weight`: (n_out + 1,) int64"""
        return np.concatenate([[0], np.cumsum(self.count, dtype=np.int64)])

    def weights_of(self, i):
        o = self.offsets
        return self.weight[o[i]:o[i + 1]]

    def c_struct(self):
        """the ebcc_hip_axis_map that points into this object's arrays (keep the object alive while it is used)"""
        return AxisMapC(self.n_out, self.first.ctypes.data, self.count.ctypes.data, self.weight.ctypes.data, int(self.wrap))


def regrid_spec(row_map, col_map):
    """the ebcc_hip_regrid_spec of two AxisMaps (which must outlive it)"""
    return RegridSpec(row_map.c_struct(), col_map.c_struct())


def _from_lists(first, weights, wrap=False):
    return AxisMap(np.asarray(first, np.int64), np.asarray([len(w) for w in weights], np.int64),
                   np.concatenate([np.asarray(w, np.float64) for w in weights]), wrap)


def identity_map(n):
    """output i is source i"""
    return AxisMap(np.arange(n), np.ones(n, np.int64), np.ones(n))


def flip_map(n):
    """output i is source n - 1 - i (a north-south flip)"""
    return AxisMap(np.arange(n)[::-1], np.ones(n, np.int64), np.ones(n))


def block_mean_map(n, k, weights=None):
    """Means over blocks of k source positions; the last block holds what is left.  weights: (n,) - lat_weights, say - that are
    normalised per block (math.fsum); None: 1 / (size of the block)."""
    n, k = int(n), int(k)
    if n < 1 or k < 1 or k > MAX_TAPS:
        raise ValueError(f"blocks of {k} over {n} positions: k must lie in 1 .. {MAX_TAPS}")
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    if w.shape != (n,):
        raise ValueError(f"weights must have the shape ({n},)")
    first = list(range(0, n, k))
    rows = []
    for f in first:
        b = w[f:f + k]
        total = math.fsum(b.tolist())
        if not total > 0 or not np.isfinite(total):
            raise ValueError(f"the weights of the block at {f} do not sum to a positive number")
        rows.append(b / total)
    return _from_lists(first, rows)


def cell_edges(centres, lo=None, hi=None):
    """The n + 1 edges of the cells around n >= 2 monotone centres: the midpoints, and half a spacing beyond the first and the
    last centre.  lo, hi: the edges are clipped to [lo, hi] - a pole-centred latitude grid takes -90, 90."""
    c = np.asarray(centres, np.float64)
    if c.ndim != 1 or c.size < 2 or not (np.all(np.diff(c) > 0) or np.all(np.diff(c) < 0)):
        raise ValueError("centres must be at least two strictly monotone numbers")
    mid = 0.5 * (c[:-1] + c[1:])
    e = np.concatenate([[c[0] - 0.5 * (c[1] - c[0])], mid, [c[-1] + 0.5 * (c[-1] - c[-2])]])
    if lo is not None or hi is not None:
        e = np.clip(e, lo, hi)
    return e


def _monotone(a, what):
    d = np.diff(a)
    if a.ndim != 1 or a.size < 2 or not np.isfinite(a).all() or not (np.all(d > 0) or np.all(d < 0)):
        raise ValueError(f"{what} must be at least two finite, strictly monotone numbers")
    return bool(d[0] < 0)


def conservative_map(src_edges, dst_edges, measure=None, period=None):
    """First-order conservative remapping along one axis: the weight of source cell k for destination cell i is the measure of
    their overlap divided by the measure of what the source covers of cell i (math.fsum), so a constant field stays that
    constant.  Edges are n + 1 strictly monotone numbers (either direction, the two grids need not agree); measure: a monotone
    function applied to the edges first - np.sin of the latitude in radians makes the measure the area of a latitude band.
    period: the axis is periodic (longitude: 360) - the source edges, increasing, span one period, destination cells are taken
    modulo the period and a cell across the seam gets a wrapping support.  ValueError for a destination cell that meets no
    source cell, and for a support of more than 256 cells."""
    s, d = np.asarray(src_edges, np.float64), np.asarray(dst_edges, np.float64)
    if measure is not None:
        s, d = np.asarray(measure(s), np.float64), np.asarray(measure(d), np.float64)
    if _monotone(s, "src_edges"):
        s, d = -s, -d                                                   # (the same cells, counted along an increasing axis)
    _monotone(d, "dst_edges")
    n = s.size - 1
    wrap = False
    if period is not None:
        if measure is not None:
            raise ValueError("a periodic axis takes no measure")
        if not np.all(np.diff(np.asarray(src_edges, np.float64)) > 0):
            raise ValueError("the source edges of a periodic axis must increase")
        period = float(period)
        if abs((s[-1] - s[0]) - period) > 1e-9 * period:
            raise ValueError("the source edges must span one period")
        s = np.concatenate([s, s[1:] + period])                         # (cell k + n is cell k one period on)
    first, rows = [], []
    for i in range(d.size - 1):
        a, b = min(d[i], d[i + 1]), max(d[i], d[i + 1])
        if period is not None:
            shift = math.floor((a - s[0]) / period) * period
            a, b = a - shift, b - shift
            if b - a > period:
                raise ValueError(f"destination cell {i} is longer than the period")
        k0 = max(int(np.searchsorted(s, a, side="right")) - 1, 0)
        k1 = min(int(np.searchsorted(s, b, side="left")), s.size - 1)   # cells k0 .. k1 - 1 may overlap
        over = np.minimum(s[k0 + 1:k1 + 1], b) - np.maximum(s[k0:k1], a)
        live = np.nonzero(over > 0)[0]
        if live.size == 0:
            raise ValueError(f"destination cell {i} meets no source cell")
        over = over[live[0]:live[-1] + 1]
        k0 += int(live[0])
        if over.size > MAX_TAPS:
            raise ValueError(f"destination cell {i} meets {over.size} source cells, more than {MAX_TAPS}")
        first.append(k0 % n)
        wrap = wrap or k0 % n + over.size > n
        rows.append(over / math.fsum(over.tolist()))
    return _from_lists(first, rows, wrap)


def linear_map(src_centres, dst_centres, period=None):
    """Linear interpolation between the two source centres around every destination centre (two taps; a destination on a source
    centre gets the weights 1 and 0).  Without a period a destination outside the source centres is a ValueError; with one the
    source centres, increasing, lie within one period and the pair across the seam is a wrapping support."""
    c, x = np.asarray(src_centres, np.float64), np.asarray(dst_centres, np.float64)
    if _monotone(c, "src_centres"):
        c, x = -c, -x
    if x.ndim != 1 or x.size < 1 or not np.isfinite(x).all():
        raise ValueError("dst_centres must be finite numbers")
    n = c.size
    wrap = False
    if period is not None:
        if not np.all(np.diff(np.asarray(src_centres, np.float64)) > 0) or c[-1] - c[0] >= period:
            raise ValueError("the source centres of a periodic axis must increase within one period")
        period = float(period)
        x = x - np.floor((x - c[0]) / period) * period
        c = np.concatenate([c, [c[0] + period]])
    elif x.min() < c[0] or x.max() > c[-1]:
        raise ValueError("a destination centre lies outside the source centres")
    k = np.clip(np.searchsorted(c, x, side="right") - 1, 0, c.size - 2)
    f = (x - c[k]) / (c[k + 1] - c[k])
    wrap = bool((k + 2 > n).any())
    return AxisMap(k, np.full(x.size, 2, np.int64), np.stack([1.0 - f, f], axis=1).ravel(), wrap)
