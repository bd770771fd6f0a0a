"""HDF5 direct-chunk batch path.

HDF5 calls a filter once per chunk (`H5Z_filter_ebcc`, /root/reference/src/h5z_ebcc.c:124-148): one frame per
call, which leaves a GPU codec launch-latency-bound.  For datasets whose chunks are single frames (1, H, W) the
chunks can instead be coded as one batch on the device and handed to HDF5 already filtered
(`H5Dwrite_chunk` / `H5Dread_chunk`, h5py's `write_direct_chunk` / `read_direct_chunk`).  The file is an ordinary
EBCC-filtered dataset: the bytes of every chunk are exactly what the filter callback would have produced, so
any HDF5 reader with the plugin on `HDF5_PLUGIN_PATH` (this build or the reference's) reads it, and files
written through the callback are read here.

Only numpy and ctypes are needed (h5py objects are passed in by the caller).
"""
import contextlib
import ctypes
import os
import sys
import threading
import time

import numpy as np

from . import load
from . import regrid as _regrid
from .filter_wrapper import EBCC_Filter, _MODES


class CodecConfig(ctypes.Structure):
    """codec_config_t, include/ebcc_codec.h (reference src/ebcc_codec.h:32-39)."""
    _fields_ = [("dims", ctypes.c_size_t * 3), ("base_cr", ctypes.c_float), ("residual_compression_type", ctypes.c_int),
                ("residual_cr", ctypes.c_float), ("error", ctypes.c_float), ("chunk_dims", ctypes.c_size_t * 3)]


def frame_config(height, width, base_cr, residual_opt=("none", None)):
    mode, value = residual_opt if residual_opt is not None else ("none", None)
    c = CodecConfig()
    c.dims[:] = (1, height, width)
    c.base_cr = base_cr
    c.residual_compression_type = _MODES[mode]
    c.residual_cr = 0.0
    c.error = float(value) if _MODES[mode] else 0.0
    c.chunk_dims[:] = (0, 0, 0)
    return c


class FrameGroup(ctypes.Structure):
    """ebcc_hip_frame_group, include/ebcc_hip.h: an array of frames with its own config."""
    _fields_ = [("frames", ctypes.c_void_p), ("n_frames", ctypes.c_size_t), ("config", CodecConfig), ("range_of_group", ctypes.c_int)]


# ebcc_hip_frame_error and ebcc_hip_bound_report, include/ebcc_hip.h, as numpy record types
FRAME_ERROR = np.dtype([("max_abs", "<f4"), ("at", "<u4"), ("n_over", "<u8"), ("sum", "<f8"), ("sum_sq", "<f8"), ("x_min", "<f4"), ("x_max", "<f4")])
BOUND_REPORT = np.dtype([("target", "<f4"), ("achieved", "<f4"), ("error_used", "<f4"), ("rounds", "<i4"), ("met", "<i4")])
assert FRAME_ERROR.itemsize == 40 and BOUND_REPORT.itemsize == 20


class TimeStats(ctypes.Structure):
    """ebcc_hip_time_stats, include/ebcc_hip.h: per-pixel accumulators [n_bins][rows][cols] on the device, count on the host."""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("d_sum", ctypes.c_void_p), ("d_sum_sq", ctypes.c_void_p), ("d_min", ctypes.c_void_p), ("d_max", ctypes.c_void_p),
                ("d_over", ctypes.c_void_p), ("threshold", ctypes.c_float), ("count", ctypes.c_void_p)]


NO_BIN = 0xFFFFFFFF                                               # EBCC_HIP_NO_BIN


class _DeviceState:
    """What the device-resident states share: the window, the arrays `fields` = [(name, dtype), ..] of `shape` on the device -
    the pointer of each is the attribute _prefix + name of the object _held() returns -, result()'s download and close()."""
    _prefix = ""

    def _held(self):
        return self.stats

    def _begin(self, codec, n, what):
        """the codec kept -> n, the number of bins or outputs (`what`: its name), 1 at least"""
        self.codec, n = codec, int(n)
        if n < 1:
            raise ValueError(f"{what} must be at least 1")
        return n

    def _open(self, n, window):
        """window, shape = (n, rows, cols) and count, n zeros -> rows, cols"""
        codec = self.codec
        self.window = (0, 0, codec.h, codec.w) if window is None else tuple(int(v) for v in window)
        row0, col0, rows, cols = self.window
        if min(row0, col0) < 0 or rows < 1 or cols < 1 or row0 + rows > codec.h or col0 + cols > codec.w:
            raise ValueError(f"window {self.window} is empty or not inside the {codec.h} x {codec.w} frame")
        self.shape = (n, rows, cols)
        self.count = np.zeros(n, np.uint64)
        return rows, cols

    def _alloc(self, init, arg=None):
        """the arrays of `fields` made on the device and set by the entry point `init` (arg: what it is given, default the
        holder of the pointers); nothing stays allocated when either fails"""
        codec, held = self.codec, self._held()
        try:
            for name, dtype in self.fields:
                p = codec.lib.ebcc_hip_malloc(int(np.prod(self.shape)) * np.dtype(dtype).itemsize)
                if not p:
                    codec._fail("ebcc_hip_malloc")
                setattr(held, self._prefix + name, p)
            if getattr(codec.lib, init)(codec.ctx, ctypes.byref(held if arg is None else arg())):
                codec._fail(init)
        except BaseException:
            self.close()
            raise

    def _download(self):
        """{name: array} of the fields"""
        got = {}
        for name, dtype in self.fields:
            a = np.empty(self.shape, dtype)
            if self.codec.lib.ebcc_hip_memcpy_d2h(a.ctypes.data, getattr(self._held(), self._prefix + name), a.nbytes):
                self.codec._fail("ebcc_hip_memcpy_d2h")
            got[name] = a
        return got

    def close(self):
        held = self._held()
        for name, _ in self.fields:
            p = getattr(held, self._prefix + name)
            if p:
                self.codec.lib.ebcc_hip_free(p)
                setattr(held, self._prefix + name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ReduceResult:
    """Statistics over time, per bin and pixel: count (n_bins,) uint64 - the frames folded into each bin -, sum and sum_sq
    (n_bins, rows, cols) float64, min and max float32, over uint32 (None without a threshold: the frames with sample >
    threshold).  The sums are those of a loop over the frames in increasing index, acc = acc + x in float64.  mean and var
    (the variance over the bin's frames, sum_sq / count - mean^2) are float64; a bin without frames gives NaN."""

    def __init__(self, count, sum, sum_sq, min, max, over):       # noqa: A002
        self.count, self.sum, self.sum_sq, self.min, self.max, self.over = count, sum, sum_sq, min, max, over

    @property
    def mean(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sum / self.count.astype(np.float64)[:, None, None]

    @property
    def var(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = self.mean
            return self.sum_sq / self.count.astype(np.float64)[:, None, None] - m * m


class ReduceState(_DeviceState):
    """The accumulators of BatchCodec.reduce, resident on the device from call to call (BatchCodec.reduce_state makes one):
    result() downloads them, close() frees them."""

    def __init__(self, codec, n_bins, window, threshold):
        self.n_bins = self._begin(codec, n_bins, "n_bins")
        rows, cols = self._open(self.n_bins, window)
        self.stats = TimeStats(self.n_bins, rows, cols, None, None, None, None, None, 0.0 if threshold is None else float(threshold),
                               self.count.ctypes.data)
        self.fields = [("d_sum", np.float64), ("d_sum_sq", np.float64), ("d_min", np.float32), ("d_max", np.float32)]
        if threshold is not None:
            self.fields.append(("d_over", np.uint32))
        self._alloc("ebcc_hip_time_stats_init")

    def result(self):
        got = self._download()
        return ReduceResult(self.count.copy(), got["d_sum"], got["d_sum_sq"], got["d_min"], got["d_max"], got.get("d_over"))


class PairStats(ctypes.Structure):
    """ebcc_hip_pair_stats, include/ebcc_hip.h: per-pixel accumulators [n_bins][rows][cols] of two variables on the device, count on the host."""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("d_sum_x", ctypes.c_void_p), ("d_sum_y", ctypes.c_void_p), ("d_sum_xx", ctypes.c_void_p), ("d_sum_yy", ctypes.c_void_p),
                ("d_sum_xy", ctypes.c_void_p), ("d_sum_mag", ctypes.c_void_p), ("d_max_mag", ctypes.c_void_p), ("d_over_mag", ctypes.c_void_p),
                ("threshold", ctypes.c_float), ("count", ctypes.c_void_p)]


class PairResult:
    """Co-moments and vector magnitude of two variables over time, per bin and pixel: count (n_bins,) uint64 - the steps folded
    into each bin -, sum_x, sum_y, sum_xx, sum_yy, sum_xy (n_bins, rows, cols) float64, and of m = sqrt(x^2 + y^2) in float32:
    sum_mag float64, max_mag float32, over_mag uint32 (the steps with m > threshold).  The magnitude arrays are None when they
    were not asked for, over_mag is None without a threshold.  The sums are those of a loop over the steps in increasing
    index, acc = acc + term in float64.  mean_x, mean_y, cov (sum_xy / n - mean_x * mean_y), corr and mean_mag are float64;
    NaN where a bin has no steps, corr also where a variance is 0."""

    def __init__(self, count, sum_x, sum_y, sum_xx, sum_yy, sum_xy, sum_mag, max_mag, over_mag):
        self.count, self.sum_x, self.sum_y, self.sum_xx, self.sum_yy, self.sum_xy = count, sum_x, sum_y, sum_xx, sum_yy, sum_xy
        self.sum_mag, self.max_mag, self.over_mag = sum_mag, max_mag, over_mag

    def _over_n(self, a):
        n = self.count.astype(np.float64)[:, None, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, a / n, np.nan)

    @property
    def mean_x(self):
        return self._over_n(self.sum_x)

    @property
    def mean_y(self):
        return self._over_n(self.sum_y)

    @property
    def cov(self):
        with np.errstate(invalid="ignore"):
            return self._over_n(self.sum_xy) - self.mean_x * self.mean_y

    @property
    def corr(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            mx, my = self.mean_x, self.mean_y
            vx, vy = self._over_n(self.sum_xx) - mx * mx, self._over_n(self.sum_yy) - my * my
            r = self.cov / np.sqrt(vx * vy)
        r[~((vx > 0) & (vy > 0))] = np.nan
        return r

    @property
    def mean_mag(self):
        return None if self.sum_mag is None else self._over_n(self.sum_mag)


class PairState(_DeviceState):
    """The accumulators of BatchCodec.pair, resident on the device from call to call (BatchCodec.pair_state makes one):
    result() downloads them, close() frees them."""

    def __init__(self, codec, n_bins, window, threshold, magnitude):
        self.n_bins = self._begin(codec, n_bins, "n_bins")
        if threshold is not None and (not magnitude or np.isnan(float(threshold))):
            raise ValueError("a threshold needs magnitude=True and must not be a NaN")
        rows, cols = self._open(self.n_bins, window)
        self.stats = PairStats(self.n_bins, rows, cols, None, None, None, None, None, None, None, None, 0.0 if threshold is None else float(threshold),
                               self.count.ctypes.data)
        self.fields = [(name, np.float64) for name in ("d_sum_x", "d_sum_y", "d_sum_xx", "d_sum_yy", "d_sum_xy")]
        if magnitude:
            self.fields += [("d_sum_mag", np.float64), ("d_max_mag", np.float32)]
        if threshold is not None:
            self.fields.append(("d_over_mag", np.uint32))
        self._alloc("ebcc_hip_pair_stats_init")

    def result(self):
        got = self._download()
        return PairResult(self.count.copy(), got["d_sum_x"], got["d_sum_y"], got["d_sum_xx"], got["d_sum_yy"], got["d_sum_xy"], got.get("d_sum_mag"),
                          got.get("d_max_mag"), got.get("d_over_mag"))


class SpellStats(ctypes.Structure):
    """ebcc_hip_spell_stats, include/ebcc_hip.h: per-pixel run, event and extreme state [n_bins][rows][cols] on the device, count on the host."""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("threshold", ctypes.c_float), ("below", ctypes.c_int), ("min_len", ctypes.c_uint32),
                ("d_run", ctypes.c_void_p), ("d_longest", ctypes.c_void_p), ("d_longest_end", ctypes.c_void_p), ("d_spells", ctypes.c_void_p),
                ("d_spell_steps", ctypes.c_void_p), ("d_events", ctypes.c_void_p), ("d_first", ctypes.c_void_p), ("d_last", ctypes.c_void_p),
                ("d_min", ctypes.c_void_p), ("d_max", ctypes.c_void_p), ("d_when_min", ctypes.c_void_p), ("d_when_max", ctypes.c_void_p),
                ("count", ctypes.c_void_p)]


NO_STEP = 0xFFFFFFFF                                              # EBCC_HIP_NO_STEP
SPELL_FAMILIES = {"runs": ("run", "longest", "longest_end", "spells", "spell_steps"), "events": ("events", "first", "last"),
                  "extremes": ("min", "max", "when_min", "when_max")}
SPELL_LABELS = ("longest_end", "first", "last", "when_min", "when_max")


class SpellResult:
    """Run lengths and event timing over time, per bin and pixel, all (n_bins, rows, cols): an event is x > threshold (below:
    x < threshold); run - the run still open after the last step -, longest - the longest run - and longest_end - the label of
    its last step, the earliest of equal runs -, spells and spell_steps - the runs of at least min_len steps and the steps that
    lie in them -; events, first and last - the count of events and the labels of the first and the last one -; min, max
    (float32), when_min and when_max - the labels of the steps that first reached them.  Everything else is uint32; a label
    nothing has set is NO_STEP.  An array that was not asked for is None.  count (n_bins,) uint64: the steps folded into each
    bin.  masked(name): a label array as a numpy masked array, masked where it is NO_STEP."""
    NAMES = SPELL_FAMILIES["runs"] + SPELL_FAMILIES["events"] + SPELL_FAMILIES["extremes"]

    def __init__(self, count, **arrays):
        self.count = count
        for name in self.NAMES:
            setattr(self, name, arrays.get(name))

    def masked(self, name):
        if name not in SPELL_LABELS:
            raise ValueError(f"{name} is not one of the label arrays {SPELL_LABELS}")
        a = getattr(self, name)
        return None if a is None else np.ma.masked_equal(a, NO_STEP)


class SpellState(_DeviceState):
    """The accumulators of BatchCodec.spells, resident on the device from call to call (BatchCodec.spell_state makes one): the
    open run of every pixel is part of them.  result() downloads them, close() frees them."""
    _prefix = "d_"

    def __init__(self, codec, threshold, below, min_len, n_bins, window, what):
        self.min_len = int(min_len)
        self.n_bins = self._begin(codec, n_bins, "n_bins")
        what = (what,) if isinstance(what, str) else tuple(what)
        if not what or any(f not in SPELL_FAMILIES for f in what):
            raise ValueError(f"what must name some of {tuple(SPELL_FAMILIES)}")
        if np.isnan(float(threshold)) and ("runs" in what or "events" in what):
            raise ValueError("the threshold must not be a NaN")
        if not 0 <= self.min_len < NO_STEP:
            raise ValueError("min_len must be a uint32")
        rows, cols = self._open(self.n_bins, window)
        self.stats = SpellStats(self.n_bins, rows, cols, float(threshold), 1 if below else 0, self.min_len)
        self.stats.count = self.count.ctypes.data
        self.fields = []
        for family in SPELL_FAMILIES:                                   # (min_len 0: there is no spell to count)
            if family in what:
                self.fields += [(name, np.float32 if name in ("min", "max") else np.uint32) for name in SPELL_FAMILIES[family]
                                if self.min_len or name not in ("spells", "spell_steps")]
        self._alloc("ebcc_hip_spell_stats_init")

    def result(self):
        return SpellResult(self.count.copy(), **self._download())


class TimeRanks(ctypes.Structure):
    """ebcc_hip_time_ranks, include/ebcc_hip.h: the order statistics asked of every bin (host) and their planes
    [n_bins][n_ranks][rows][cols] (device), count on the host."""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t), ("n_ranks", ctypes.c_size_t),
                ("rank", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("count", ctypes.c_void_p)]


NO_RANK = 2 ** 64 - 1                                             # EBCC_HIP_NO_RANK
MAX_RANKS = 16                                                    # EBCC_HIP_MAX_RANKS
QUANTILE_METHODS = ("linear", "lower", "higher", "nearest")


def quantile_rule(q, m, method="linear"):
    """The rank rule of BatchCodec.quantiles for a bin of m >= 1 frames, in float64: h = q * (m - 1) -> (lo, hi, t), the
    quantile being lo_value + (hi_value - lo_value) * t of the order statistics at the 0-based ranks lo and hi.  `lower`:
    floor(h); `higher`: ceil(h); `nearest`: h rounded half to even; `linear`: floor(h), ceil(h) and t = h - floor(h).  All but
    `linear` give lo == hi and t == 0."""
    if method not in QUANTILE_METHODS:
        raise ValueError(f"method must be one of {QUANTILE_METHODS}, got {method!r}")
    q = np.float64(q)
    if not (q >= 0.0 and q <= 1.0):
        raise ValueError(f"a quantile must lie in [0, 1], got {q}")
    if m < 1:
        raise ValueError("a bin without frames has no quantile")
    h = q * np.float64(m - 1)
    fl, ce = int(np.floor(h)), int(np.ceil(h))
    if method == "lower":
        return fl, fl, np.float64(0.0)
    if method == "higher":
        return ce, ce, np.float64(0.0)
    if method == "nearest":
        r = int(np.rint(h))
        return r, r, np.float64(0.0)
    return fl, ce, h - np.floor(h)


class QuantileResult:
    """Quantiles over time, per bin and pixel: values (n_bins, len(q), rows, cols) float32 and count (n_bins,) uint64 - the
    frames of each bin.  A bin without frames gives NaN planes."""

    def __init__(self, values, count):
        self.values, self.count = values, count


class TimeMap(ctypes.Structure):
    """ebcc_hip_time_map, include/ebcc_hip.h: the terms of every output as CSR arrays (host), the accumulators
    [n_out][rows][cols] of doubles (device), count on the host."""
    _fields_ = [("n_out", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t), ("start", ctypes.c_void_p),
                ("frame", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("d_acc", ctypes.c_void_p), ("count", ctypes.c_void_p)]


def time_map_terms(weights, n_frames=None):
    """The CSR arrays of a time map -> (start uint64 (n_out + 1,), frame uint32 (n_terms,), weight float64 (n_terms,)): output
    o owns the terms start[o] .. start[o + 1).  `weights`: a dense array [n_out][n_frames] of any real dtype, converted to
    float64 - entries equal to 0 are dropped, the others become the terms of their row in increasing frame -, or a triple
    (start, frame, weight), used as given.  n_frames: the length of the frame axis (a dense array's own).  ValueError for what
    ebcc_hip_time_map_check would refuse of these arrays: start[0] != 0, a decreasing start, no term at all, a frame >=
    n_frames, frames not strictly increasing within an output, a NaN or Inf weight."""
    if isinstance(weights, tuple) and len(weights) == 3:
        start, frame, weight = (np.asarray(v) for v in weights)
        if start.ndim != 1 or start.size < 2 or start.dtype.kind not in "iu" or (start.astype(np.int64) < 0).any():
            raise ValueError("start must be n_out + 1 integers that are not negative, n_out >= 1")
        if frame.ndim != 1 or frame.dtype.kind not in "iu" or (frame.size and (frame.astype(np.int64).min() < 0 or frame.astype(np.int64).max() >= 2 ** 32)):
            raise ValueError("frame must be integers that fit 32 bits")
        if weight.ndim != 1 or weight.dtype.kind not in "fiu":
            raise ValueError("weight must be real numbers")
        start, frame, weight = start.astype(np.uint64), frame.astype(np.uint32), weight.astype(np.float64)
    else:
        dense = np.asarray(weights)
        if dense.ndim != 2 or dense.shape[0] < 1 or dense.dtype.kind not in "fiu":
            raise ValueError("weights must be a real array [n_out][n_frames] or a (start, frame, weight) triple")
        dense = dense.astype(np.float64)
        if n_frames is not None and int(n_frames) != dense.shape[1]:
            raise ValueError(f"the frame axis of weights has {dense.shape[1]} entries, not {n_frames}")
        n_frames = dense.shape[1]
        out, at = np.nonzero(dense != 0.0)                          # (row-major: increasing frame within an output; NaN != 0)
        start = np.concatenate([[0], np.cumsum(np.bincount(out, minlength=dense.shape[0]))]).astype(np.uint64)
        frame, weight = at.astype(np.uint32), dense[out, at]
    if start[0] != 0:
        raise ValueError("start[0] must be 0")
    if (np.diff(start.astype(np.int64)) < 0).any():
        raise ValueError("start decreases")
    n_terms = int(start[-1])
    if n_terms < 1:
        raise ValueError("no term at all")
    if frame.size < n_terms or weight.size < n_terms:
        raise ValueError(f"start names {n_terms} terms, frame has {frame.size} and weight {weight.size}")
    frame, weight = np.ascontiguousarray(frame[:n_terms]), np.ascontiguousarray(weight[:n_terms])
    if n_frames is not None and int(frame.max()) >= int(n_frames):
        raise ValueError(f"a term names frame {int(frame.max())} of {int(n_frames)}")
    inner = np.ones(n_terms, bool)                                  # terms that have a predecessor in their output
    inner[start[:-1][start[:-1] < n_terms].astype(np.int64)] = False
    if (np.diff(frame.astype(np.int64)) <= 0)[inner[1:]].any():
        raise ValueError("the frames of an output must be strictly increasing")
    if not np.isfinite(weight).all():
        raise ValueError("every weight must be finite")
    return np.ascontiguousarray(start), frame, weight


def trend_weights(times):
    """The 2 x n time map of the least-squares line through n >= 2 samples at `times` (float64): row 0 is 1 / n - the mean -,
    row 1 is (t - mean(t)) / sum((t - mean(t))^2) - the slope per unit of `times`.  Plain float64 numpy."""
    t = np.asarray(times, np.float64)
    if t.ndim != 1 or t.size < 2 or not np.isfinite(t).all():
        raise ValueError("times must be at least two finite numbers")
    c = t - t.mean()
    ss = (c * c).sum()
    if not ss > 0.0:
        raise ValueError("times must not all be equal")
    return np.stack([np.full(t.size, 1.0 / t.size), c / ss])


def running_mean_weights(n, width):
    """The banded (n - width + 1) x n time map of the running mean over `width` consecutive frames: output o has the weight
    1 / width at the frames o .. o + width - 1 and 0 elsewhere.  Plain float64 numpy."""
    n, width = int(n), int(width)
    if width < 1 or width > n:
        raise ValueError("width must lie in [1, n]")
    w = np.zeros((n - width + 1, n), np.float64)
    for o in range(n - width + 1):
        w[o, o:o + width] = 1.0 / width
    return w


class ProjectResult:
    """Weighted sums over time, per output and pixel: values (n_out, rows, cols) float64 - for every output the bytes of a loop
    over its terms in increasing frame, acc = acc + weight * float64(x) - and count (n_out,) uint64, the terms folded into
    each output."""

    def __init__(self, values, count):
        self.values, self.count = values, count


class MapState(_DeviceState):
    """The accumulators of BatchCodec.project, resident on the device from call to call (BatchCodec.map_state makes one):
    result() downloads them, close() frees them."""

    def _held(self):
        return self

    def __init__(self, codec, n_out, window):
        self.n_out = self._begin(codec, n_out, "n_out")
        self._open(self.n_out, window)
        self.d_acc, self.fields = None, [("d_acc", np.float64)]
        self._alloc("ebcc_hip_time_map_init", lambda: self.map(None, None, None))

    def map(self, start, frame, weight):
        """the ebcc_hip_time_map of these accumulators with the terms of one call (arrays the caller keeps alive)"""
        return TimeMap(self.n_out, self.shape[1], self.shape[2], *(None if a is None else a.ctypes.data for a in (start, frame, weight)),
                       self.d_acc, self.count.ctypes.data)

    def result(self):
        return ProjectResult(self._download()["d_acc"], self.count.copy())


def _terms_of_range(terms, lo, hi):
    """the terms of the CSR triple whose frame lies in [lo, hi), frames rebased to lo -> a triple (n_terms may be 0)"""
    start, frame, weight = terms
    keep = (frame >= lo) & (frame < hi)
    owner = np.repeat(np.arange(len(start) - 1), np.diff(start.astype(np.int64)))
    part = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=len(start) - 1))]).astype(np.uint64)
    return part, (frame[keep].astype(np.int64) - lo).astype(np.uint32), np.ascontiguousarray(weight[keep])


class Region(ctypes.Structure):
    """ebcc_hip_region, include/ebcc_hip.h: a box of a frame"""
    _fields_ = [("row0", ctypes.c_size_t), ("col0", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t)]


class AreaSpec(ctypes.Structure):
    """ebcc_hip_area_spec, include/ebcc_hip.h: the regions, the row weights (host) and the pixel weights (device) of an area series"""
    _fields_ = [("n_regions", ctypes.c_size_t), ("regions", ctypes.POINTER(Region)), ("w_row", ctypes.c_void_p), ("d_w_pix", ctypes.c_void_p),
                ("use_threshold", ctypes.c_int), ("threshold", ctypes.c_float)]


# ebcc_hip_area_stat, include/ebcc_hip.h, as a numpy record type
AREA_STAT = np.dtype([("sum", "<f8"), ("sum_sq", "<f8"), ("over", "<f8"), ("min", "<f4"), ("max", "<f4")])
assert AREA_STAT.itemsize == 32


class SeriesResult:
    """Statistics over regions, per frame and region: sum, sum_sq and over (n, R) float64 - the weighted sums of x and x^2 and
    the weight of the pixels with x > threshold (zeros without one) -, min and max (n, R) float32 over the pixels of non-zero
    weight, weight (R,) float64: the total weight of each region (math.fsum: order-free).  The sums are those of the fold
    include/ebcc_hip.h states, whatever the engine's capacity.  mean = sum / weight and var = sum_sq / weight - mean^2 are
    float64; a region without weight gives NaN."""

    def __init__(self, records, weight):
        self.sum, self.sum_sq, self.over = (np.ascontiguousarray(records[name]) for name in ("sum", "sum_sq", "over"))
        self.min, self.max = np.ascontiguousarray(records["min"]), np.ascontiguousarray(records["max"])
        self.weight = weight

    @property
    def mean(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sum / self.weight[None, :]

    @property
    def var(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = self.mean
            return self.sum_sq / self.weight[None, :] - m * m


def lat_weights(lat_degrees):
    """cos(latitude) in float64: the row weights of an area mean on a regular latitude-longitude grid"""
    return np.cos(np.deg2rad(np.asarray(lat_degrees, np.float64)))


class _Area:
    """The checked arguments of an area series: the region table, the row weights and - uploaded once, freed by close() - the
    pixel weights on the device, as the ebcc_hip_area_spec the calls take."""

    def __init__(self, codec, regions, w_row, w_pix, threshold):
        h, w = codec.h, codec.w
        r = np.asarray(regions)
        if r.ndim != 2 or r.shape[1] != 4 or r.shape[0] < 1 or r.dtype.kind not in "iu":
            raise ValueError("regions must be a non-empty integer array of shape (R, 4): row0, col0, rows, cols")
        r = r.astype(np.int64)
        if (r[:, :2] < 0).any() or (r[:, 2:] < 1).any() or (r[:, 0] + r[:, 2] > h).any() or (r[:, 1] + r[:, 3] > w).any():
            raise ValueError(f"a region is empty or not inside the {h} x {w} frame")
        self.codec, self.regions = codec, r
        self.table = (Region * len(r))(*[Region(*(int(v) for v in row)) for row in r])
        self.w_row = None if w_row is None else np.ascontiguousarray(w_row, np.float64)
        if self.w_row is not None and (self.w_row.shape != (h,) or not np.isfinite(self.w_row).all() or (self.w_row < 0).any()):
            raise ValueError(f"w_row must be {h} finite weights that are not negative")
        self.w_pix = None if w_pix is None else np.ascontiguousarray(w_pix, np.float32)
        if self.w_pix is not None and self.w_pix.shape != (h, w):
            raise ValueError(f"w_pix must have the shape ({h}, {w})")
        self.d_w_pix = None
        if self.w_pix is not None:
            self.d_w_pix = codec.lib.ebcc_hip_malloc(self.w_pix.nbytes)
            if not self.d_w_pix:
                codec._fail("ebcc_hip_malloc")
            if codec.lib.ebcc_hip_memcpy_h2d(self.d_w_pix, self.w_pix.ctypes.data, self.w_pix.nbytes):
                self.close()
                codec._fail("ebcc_hip_memcpy_h2d")
        self.spec = AreaSpec(len(r), self.table, None if self.w_row is None else self.w_row.ctypes.data, self.d_w_pix,
                             0 if threshold is None else 1, 0.0 if threshold is None else float(threshold))

    def weight(self):
        """the total weight of every region, order-free"""
        import math
        out = np.empty(len(self.regions), np.float64)
        for g, (row0, col0, rows, cols) in enumerate(self.regions):
            wr = np.ones(rows, np.float64) if self.w_row is None else self.w_row[row0:row0 + rows]
            if self.w_pix is None:
                out[g] = math.fsum(np.repeat(wr, cols).tolist()) if self.w_row is not None else float(rows * cols)
            else:
                out[g] = math.fsum((wr[:, None] * self.w_pix[row0:row0 + rows, col0:col0 + cols].astype(np.float64)).ravel().tolist())
        return out

    def run(self, streams):
        """the records (n, R) of the streams"""
        n = len(streams)
        if n < 1:
            raise ValueError("no streams")
        streams, ptrs, sizes = _stream_arrays(streams)
        records = np.zeros((n, len(self.regions)), AREA_STAT)
        if self.codec.lib.ebcc_hip_series_shard(self.codec.ctx, ptrs, sizes, n, ctypes.byref(self.spec), records.ctypes.data):
            self.codec._fail("ebcc_hip_series_shard")
        return records

    def close(self):
        if self.d_w_pix:
            self.codec.lib.ebcc_hip_free(self.d_w_pix)
            self.d_w_pix = None


class BoundNotMet(RuntimeError):
    """A hard-bound write found frames that stay over their bound (return value 3 of the _hard entry points); `report` is
    the BOUND_REPORT array of the call that found them.  Nothing of that call has been written."""

    def __init__(self, message, report):
        super().__init__(message)
        self.report = report


def _stream_arrays(streams, named=None):
    """(the streams as bytes - the caller keeps them alive for the call -, their ctypes pointer array, their size array);
    `named`: only the streams at these indices are read, the others (None allowed) become a null pointer of size 0"""
    n = len(streams)
    kept = [None if named is not None and i not in named else (s if isinstance(s, bytes) else bytes(s)) for i, s in enumerate(streams)]
    ptrs = (ctypes.c_void_p * n)(*[None if s is None else ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p).value for s in kept])
    sizes = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in kept])
    return kept, ptrs, sizes


def _box_array(boxes):
    """`boxes` as an int64 array (k, 3) of (frame, row0, col0)"""
    b = np.asarray(boxes)
    if b.ndim != 2 or b.shape[1] != 3 or b.shape[0] < 1 or b.dtype.kind not in "iu":
        raise ValueError("boxes must be a non-empty integer array of shape (k, 3): frame, row0, col0")
    return b.astype(np.int64)


def _bin_table(bins, n, n_bins, per, none_named):
    """`bins` of a call over n streams or steps (None: all bin 0, -1: skipped) -> (b, table): the bins as int64 and the uint32
    table the engine takes, NO_BIN where one is skipped.  ValueError with the texts of the call: `per` - "stream" / "step" -
    and none_named, the message when every entry is skipped."""
    b = np.zeros(n, np.int64) if bins is None else np.asarray(bins)
    if n < 1 or b.shape != (n,) or b.dtype.kind not in "iu":
        raise ValueError(f"bins must be {n} integers, one per {per}")
    b = b.astype(np.int64)
    if b.min() < -1 or b.max() >= n_bins:
        raise ValueError(f"bins must lie in [-1, {n_bins})")
    if not (b >= 0).any():
        raise ValueError(none_named)
    return b, np.where(b < 0, NO_BIN, b).astype(np.uint32)


def _read_chunks(dset, frames):
    """The raw chunks of the frames `frames` (counted in C order over the leading axes) of a one-frame-per-chunk dataset"""
    lead = dset.shape[:-2]
    raw = []
    for f in frames:
        idx = np.unravel_index(int(f), lead) if lead else ()
        mask, chunk = dset.id.read_direct_chunk(tuple(int(v) for v in idx) + (0, 0))
        if mask:
            raise ValueError(f"chunk {idx} was stored with filters disabled (mask {mask})")
        raw.append(chunk)
    return raw


class BatchCodec:
    """Device engine for stacks of (H, W) float32 frames held in host memory."""

    def __init__(self, height, width, max_frames=256, device=0):
        lib = self.lib = load()
        lib.ebcc_hip_create.restype = ctypes.c_void_p
        lib.ebcc_hip_create.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]
        lib.ebcc_hip_destroy.argtypes = [ctypes.c_void_p]
        lib.ebcc_hip_malloc.restype = ctypes.c_void_p
        lib.ebcc_hip_malloc.argtypes = [ctypes.c_size_t]
        lib.ebcc_hip_free.argtypes = [ctypes.c_void_p]
        lib.ebcc_hip_memcpy_h2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        lib.ebcc_hip_memcpy_d2h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        lib.ebcc_hip_encode_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(CodecConfig),
                                               ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        lib.ebcc_hip_decode_frames.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                               ctypes.c_size_t, ctypes.c_void_p]
        lib.ebcc_hip_upload.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        lib.ebcc_hip_download.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        lib.ebcc_hip_encode_host_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(CodecConfig),
                                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        lib.ebcc_hip_decode_host_frames.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                                    ctypes.c_size_t, ctypes.c_void_p]
        lib.ebcc_hip_decode_host_frames_window.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                                           ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                           ctypes.c_void_p]
        lib.ebcc_hip_decode_host_frames_boxes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                                          ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                          ctypes.c_void_p]
        lib.ebcc_hip_decode_host_frames_placed.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                                           ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        lib.ebcc_hip_encode_host_frames_groups.argtypes = [ctypes.c_void_p, ctypes.POINTER(FrameGroup), ctypes.c_size_t,
                                                           ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        lib.ebcc_hip_encode_host_frames_hard.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(CodecConfig), ctypes.c_int,
                                                         ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
        lib.ebcc_hip_encode_host_frames_groups_hard.argtypes = [ctypes.c_void_p, ctypes.POINTER(FrameGroup), ctypes.c_size_t, ctypes.c_int,
                                                                ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
        lib.ebcc_hip_audit_host_frames.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                                   ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.ebcc_hip_time_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(TimeStats)]
        lib.ebcc_hip_reduce_shard.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(TimeStats)]
        lib.ebcc_hip_pair_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(PairStats)]
        lib.ebcc_hip_pair_shard.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                            ctypes.POINTER(PairStats)]
        lib.ebcc_hip_spell_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(SpellStats)]
        lib.ebcc_hip_spell_shard.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(SpellStats)]
        lib.ebcc_hip_series_shard.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                              ctypes.POINTER(AreaSpec), ctypes.c_void_p]
        lib.ebcc_hip_quantile_shard.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(TimeRanks)]
        lib.ebcc_hip_time_map_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(TimeMap)]
        lib.ebcc_hip_project_shard.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                               ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(TimeMap)]
        for name in ("ebcc_hip_regrid_shard", "ebcc_hip_regrid_host_frames"):
            getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                           ctypes.POINTER(_regrid.RegridSpec), ctypes.c_void_p]
        lib.ebcc_hip_regrid_check.restype = ctypes.c_long
        lib.ebcc_hip_regrid_check.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_regrid.RegridSpec), ctypes.c_void_p]
        lib.ebcc_hip_last_error.restype = ctypes.c_char_p
        lib.free_buffer.argtypes = [ctypes.c_void_p]
        self.h, self.w, self.max_frames = int(height), int(width), int(max_frames)
        self.ctx = lib.ebcc_hip_create(device, self.max_frames, self.h, self.w)
        if not self.ctx:
            self._fail("EBCC MI355X engine")

    def _fail(self, name):
        raise RuntimeError(name + ": " + (self.lib.ebcc_hip_last_error() or b"?").decode())

    def close(self):
        if self.ctx:
            self.lib.ebcc_hip_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def encode(self, frames, cfg, hard=False, max_rounds=0):
        """frames: (n, H, W) float32 in host memory, any n -> list of EBCC frame streams (bytes).  More frames than the
        engine holds are coded in batches on two alternating engine sets (the host part of one batch beside the upload and
        the kernels of the next).  hard=True: every batch is audited on the device and the frames over their bound are coded
        again with a smaller error, at most max_rounds times (0: 6) - ebcc_hip_encode_host_frames_hard; the result is then
        (streams, report), report a BOUND_REPORT array with one record per frame (met == 0: still over its bound)."""
        frames = np.ascontiguousarray(frames, np.float32)
        n = frames.shape[0]
        assert frames.shape[1:] == (self.h, self.w) and n >= 1
        outs = (ctypes.c_void_p * n)()
        sizes = (ctypes.c_size_t * n)()
        report = np.zeros(n, BOUND_REPORT)
        if hard:
            if self.lib.ebcc_hip_encode_host_frames_hard(self.ctx, frames.ctypes.data, n, ctypes.byref(cfg), int(max_rounds), outs, sizes,
                                                         report.ctypes.data) not in (0, 3):
                self._fail("ebcc_hip_encode_host_frames_hard")
        elif self.lib.ebcc_hip_encode_host_frames(self.ctx, frames.ctypes.data, n, ctypes.byref(cfg), outs, sizes):
            self._fail("ebcc_hip_encode_host_frames")
        res = []
        for i in range(n):
            res.append(ctypes.string_at(outs[i], sizes[i]))
            self.lib.free_buffer(outs[i])
        return (res, report) if hard else res

    def audit(self, streams, frames, bound=None):
        """What a reader of `streams` gets against the originals `frames` ((n, H, W) float32 in host memory, any n), measured on
        the device -> a FRAME_ERROR array with one record per frame: max_abs and the pixel `at` which it occurs, n_over (pixels
        with |x - x^| > bound[frame]; `bound`: a float or n floats, None: not counted), sum and sum_sq of x - x^, x_min and
        x_max.  No decoded frame comes back.  ValueError for NaN / Inf in the originals, RuntimeError for what the decode
        refuses."""
        n = len(streams)
        frames = np.ascontiguousarray(frames, np.float32)
        if n < 1 or frames.shape != (n, self.h, self.w):
            raise ValueError(f"{n} streams need originals of shape ({n}, {self.h}, {self.w}), got {frames.shape}")
        streams, ptrs, sizes = _stream_arrays(streams)
        b = None if bound is None else np.ascontiguousarray(np.broadcast_to(np.asarray(bound, np.float32), (n,)))
        report = np.zeros(n, FRAME_ERROR)
        rc = self.lib.ebcc_hip_audit_host_frames(self.ctx, ptrs, sizes, n, frames.ctypes.data, None if b is None else b.ctypes.data,
                                                 report.ctypes.data)
        if rc == 2:
            raise ValueError("NaN or Inf in the originals")
        if rc:
            self._fail("ebcc_hip_audit_host_frames")
        return report

    def reduce_state(self, n_bins=1, window=None, threshold=None):
        """Device-resident accumulators for reduce(state=...): n_bins bins of the window (row0, col0, rows, cols) - None: the
        whole frame -, with an exceedance count when a threshold is given.  A ReduceState; close() it when done."""
        return ReduceState(self, n_bins, window, threshold)

    def reduce(self, streams, bins=None, n_bins=1, window=None, threshold=None, state=None):
        """Statistics over time straight from the streams (ebcc_hip_reduce_shard): every frame - or its `window` = (row0, col0,
        rows, cols), decoded from the code-blocks it depends on alone - is folded on the device into the accumulators of the
        bin `bins` names for it (an integer per stream, None: all bin 0, -1: the frame is skipped and not read - its entry of
        `streams` may be None) -> a ReduceResult.  No decoded frame leaves the device; the sums are the bytes of a loop over
        the frames in order, whatever the engine's capacity.  `state`: a ReduceState (reduce_state) that is added to and
        returned instead - n_bins, window and threshold are then the state's -, so that a series walked call by call in frame
        order gives the bytes of one call; state.result() downloads the accumulators.  ValueError for bins the engine refuses,
        RuntimeError for what the call reports, such as a malformed stream (the state must then be made anew)."""
        n = len(streams)
        own = state is None
        if own:
            state = ReduceState(self, n_bins, window, threshold)
        try:
            b, table = _bin_table(bins, n, state.n_bins, "stream", "no frame is named")
            streams, ptrs, sizes = _stream_arrays(streams, named=set(int(f) for f in np.nonzero(b >= 0)[0]))
            row0, col0 = state.window[:2]
            if self.lib.ebcc_hip_reduce_shard(self.ctx, ptrs, sizes, n, table.ctypes.data, row0, col0, ctypes.byref(state.stats)):
                self._fail("ebcc_hip_reduce_shard")
            return state.result() if own else state
        finally:
            if own:
                state.close()

    def pair_state(self, n_bins=1, window=None, threshold=None, magnitude=True):
        """Device-resident accumulators for pair(state=...): n_bins bins of the window (row0, col0, rows, cols) - None: the
        whole frame -, the magnitude's sum and maximum unless magnitude=False, its exceedance count when a threshold is given.
        A PairState; close() it when done."""
        return PairState(self, n_bins, window, threshold, magnitude)

    def pair(self, streams_x, streams_y, bins=None, n_bins=1, window=None, threshold=None, magnitude=True, state=None):
        """Co-moments and vector magnitude of two variables over time straight from the streams (ebcc_hip_pair_shard): step t
        pairs streams_x[t] with streams_y[t] - frames of the engine's geometry, or their `window` = (row0, col0, rows, cols) -,
        and every step is folded on the device into the accumulators of the bin `bins` names for it (an integer per step,
        None: all bin 0, -1: the step is skipped and not read - its entries may be None) -> a PairResult.  No decoded frame
        leaves the device; the sums are the bytes of a loop over the steps in order, whatever the engine's capacity (2 at the
        least).  streams_x may be streams_y.  `state`: a PairState (pair_state) that is added to and returned instead - n_bins,
        window, threshold and magnitude are then the state's -, so that a series walked call by call in step order gives the
        bytes of one call.  ValueError for bins the engine refuses, RuntimeError for what the call reports, such as a
        malformed stream (the state must then be made anew)."""
        n = len(streams_x)
        if len(streams_y) != n:
            raise ValueError(f"{n} streams of x and {len(streams_y)} of y")
        own = state is None
        if own:
            state = PairState(self, n_bins, window, threshold, magnitude)
        try:
            b, table = _bin_table(bins, n, state.n_bins, "step", "no step is named")
            named = set(int(f) for f in np.nonzero(b >= 0)[0])
            keep_x, ptrs_x, sizes_x = _stream_arrays(streams_x, named=named)
            keep_y, ptrs_y, sizes_y = (keep_x, ptrs_x, sizes_x) if streams_y is streams_x else _stream_arrays(streams_y, named=named)
            row0, col0 = state.window[:2]
            if self.lib.ebcc_hip_pair_shard(self.ctx, ptrs_x, sizes_x, ptrs_y, sizes_y, n, table.ctypes.data, row0, col0, ctypes.byref(state.stats)):
                self._fail("ebcc_hip_pair_shard")
            return state.result() if own else state
        finally:
            if own:
                state.close()

    def spell_state(self, threshold, below=False, min_len=1, n_bins=1, window=None, what=("runs", "events", "extremes")):
        """Device-resident accumulators for spells(state=...): n_bins bins of the window (row0, col0, rows, cols) - None: the
        whole frame - with the arrays of the families `what` names.  A SpellState; close() it when done."""
        return SpellState(self, threshold, below, min_len, n_bins, window, what)

    def spells(self, streams, threshold, below=False, min_len=1, bins=None, when=None, fresh=None, n_bins=1, window=None,
               what=("runs", "events", "extremes"), state=None):
        """Run lengths and event timing over time straight from the streams (ebcc_hip_spell_shard): every frame - or its
        `window` = (row0, col0, rows, cols) - is a step, folded on the device in step order into the state of the bin `bins`
        names for it (an integer per stream, None: all bin 0, -1: the step is skipped and not read - its entry of `streams` may
        be None) -> a SpellResult.  A sample is an event where x > threshold (below=True: x < threshold); `when`: the label of
        every step, a uint32 below NO_STEP (None: its index in `streams`); `fresh`: true at the first step of every visit to a
        bin that recurs - the run does not continue from the visit before; min_len: the length from which a run is a spell (0:
        spells are not counted); `what`: the families to compute, of "runs", "events", "extremes".  No decoded frame leaves the
        device; the arrays are the bytes of a loop over the steps in order, whatever the engine's capacity.  `state`: a
        SpellState (spell_state) that is continued and returned instead - threshold, below, min_len, n_bins, window and what
        are then the state's -, so that a series walked call by call in step order gives the bytes of one call, runs that cross
        the calls included (give `when`: the default labels start at 0 in every call).  ValueError for bins or labels the engine
        refuses, RuntimeError for what the call reports, such as a malformed stream (the state must then be made anew)."""
        n = len(streams)
        own = state is None
        if own:
            state = SpellState(self, threshold, below, min_len, n_bins, window, what)
        try:
            b, table = _bin_table(bins, n, state.n_bins, "stream", "no step is named")
            labels = None
            if when is not None:
                labels = np.asarray(when)
                if labels.shape != (n,) or labels.dtype.kind not in "iu" or labels.min() < 0 or labels[b >= 0].max() >= NO_STEP or labels.max() > NO_STEP:
                    raise ValueError(f"when must be {n} integers in [0, {NO_STEP}), one per stream")
                labels = np.ascontiguousarray(labels, np.uint32)
            flags = None
            if fresh is not None:
                flags = np.ascontiguousarray(np.asarray(fresh).astype(bool), np.uint8)
                if flags.shape != (n,):
                    raise ValueError(f"fresh must be {n} flags, one per stream")
            streams, ptrs, sizes = _stream_arrays(streams, named=set(int(f) for f in np.nonzero(b >= 0)[0]))
            row0, col0 = state.window[:2]
            if self.lib.ebcc_hip_spell_shard(self.ctx, ptrs, sizes, n, table.ctypes.data, None if labels is None else labels.ctypes.data,
                                             None if flags is None else flags.ctypes.data, row0, col0, ctypes.byref(state.stats)):
                self._fail("ebcc_hip_spell_shard")
            return state.result() if own else state
        finally:
            if own:
                state.close()

    def quantiles(self, streams, q, bins=None, n_bins=1, window=None, method="linear"):
        """Quantiles over time straight from the streams (ebcc_hip_quantile_shard): for every bin - `bins` as in reduce: an
        integer per stream, None: all bin 0, -1: the frame is skipped and not read - and every q of the sequence `q` (each in
        [0, 1]) the quantile at every pixel of the frame or of its `window` = (row0, col0, rows, cols) -> a QuantileResult.
        The device selects order statistics - samples that occur, by a radix select over eight decodes of the series, with
        -0 as +0 and NaN last -; the rank rule runs here in float64 (quantile_rule): for a bin of m frames h = q (m - 1), and
        `lower`, `higher`, `nearest` (half to even) return the order statistic at that rank, `linear` float32(lo + (hi - lo)
        (h - floor(h))) computed in float64 from the two around h (the order statistic itself where h is whole).  The distinct
        ranks a bin needs go to the device once, at most 16 per call: ValueError with the number above that, and for a q
        outside [0, 1], an unknown method or bins the engine refuses; RuntimeError for what the call reports."""
        n = len(streams)
        qs = np.atleast_1d(np.asarray(q, np.float64))
        if qs.ndim != 1 or qs.size < 1:
            raise ValueError("q must be a number or a non-empty sequence of numbers")
        if method not in QUANTILE_METHODS:
            raise ValueError(f"method must be one of {QUANTILE_METHODS}, got {method!r}")
        if not ((qs >= 0.0) & (qs <= 1.0)).all():
            raise ValueError(f"every quantile must lie in [0, 1], got {qs.tolist()}")
        n_bins = int(n_bins)
        row0, col0, rows, cols = (0, 0, self.h, self.w) if window is None else tuple(int(v) for v in window)
        if n_bins < 1 or min(row0, col0) < 0 or rows < 1 or cols < 1 or row0 + rows > self.h or col0 + cols > self.w:
            raise ValueError(f"n_bins {n_bins} or window {(row0, col0, rows, cols)} does not fit the {self.h} x {self.w} frame")
        b, table = _bin_table(bins, n, n_bins, "stream", "no frame is named")
        m = np.bincount(b[b >= 0], minlength=n_bins)
        rules = [[quantile_rule(v, int(m[k]), method) for v in qs] if m[k] else None for k in range(n_bins)]
        slots = [sorted({r for lo, hi, _ in rule for r in (lo, hi)}) if rule else [] for rule in rules]
        n_ranks = max(len(s) for s in slots)
        if n_ranks > MAX_RANKS:
            raise ValueError(f"a bin needs {n_ranks} distinct ranks, more than the {MAX_RANKS} of one call")
        rank = np.full((n_bins, n_ranks), NO_RANK, np.uint64)
        for k, s in enumerate(slots):
            rank[k, :len(s)] = s
        count = np.zeros(n_bins, np.uint64)
        planes = np.empty((n_bins, n_ranks, rows, cols), np.float32)
        streams, ptrs, sizes = _stream_arrays(streams, named=set(int(f) for f in np.nonzero(b >= 0)[0]))
        d_out = self.lib.ebcc_hip_malloc(planes.nbytes)
        if not d_out:
            self._fail("ebcc_hip_malloc")
        try:
            spec = TimeRanks(n_bins, rows, cols, n_ranks, rank.ctypes.data, d_out, count.ctypes.data)
            if self.lib.ebcc_hip_quantile_shard(self.ctx, ptrs, sizes, n, table.ctypes.data, row0, col0, ctypes.byref(spec)):
                self._fail("ebcc_hip_quantile_shard")
            if self.lib.ebcc_hip_memcpy_d2h(planes.ctypes.data, d_out, planes.nbytes):
                self._fail("ebcc_hip_memcpy_d2h")
        finally:
            self.lib.ebcc_hip_free(d_out)
        values = np.full((n_bins, len(qs), rows, cols), np.nan, np.float32)
        for k, rule in enumerate(rules):
            for i, (lo, hi, t) in enumerate(rule or ()):
                low = planes[k, slots[k].index(lo)]
                if hi == lo:
                    values[k, i] = low
                else:
                    low64, high64 = low.astype(np.float64), planes[k, slots[k].index(hi)].astype(np.float64)
                    with np.errstate(invalid="ignore", over="ignore"):
                        values[k, i] = (low64 + (high64 - low64) * t).astype(np.float32)
        return QuantileResult(values, count)

    def map_state(self, n_out, window=None):
        """Device-resident accumulators for project(state=...): n_out outputs of the window (row0, col0, rows, cols) - None:
        the whole frame -, set to 0.  A MapState; close() it when done."""
        return MapState(self, n_out, window)

    def project(self, streams, weights, window=None, state=None, first=0):
        """Weighted sums over time straight from the streams (ebcc_hip_project_shard): for every output o of the time map
        `weights` - a dense [n_out][n_frames] array or a (start, frame, weight) triple, see time_map_terms - and every pixel of
        the frame or of its `window` = (row0, col0, rows, cols) the sum of weight * x over the output's terms, folded on the
        device in increasing frame: acc = acc + weight * float64(x), product and sum each rounded to float64 -> a
        ProjectResult.  `first` is the index streams[0] has on the frame axis of `weights`; terms outside [first, first +
        len(streams)) belong to other calls.  A stream no term names is not read and may be None.  No decoded frame leaves the
        device, and the sums are the bytes of that loop whatever the engine's capacity.  `state`: a MapState (map_state) that
        is added to and returned instead - the window is then the state's -, so that a series walked call by call in frame
        order gives the bytes of one call; state.result() downloads the accumulators.  ValueError for a map the engine would
        refuse or one without a term in this call, RuntimeError for what the call reports, such as a malformed stream (the
        state must then be made anew)."""
        n, first = len(streams), int(first)
        terms = time_map_terms(weights)
        if n < 1 or first < 0:
            raise ValueError("streams must not be empty and first must not be negative")
        start, frame, weight = _terms_of_range(terms, first, first + n)
        if not len(frame):
            raise ValueError(f"no term names a frame in [{first}, {first + n})")
        own = state is None
        if own:
            state = MapState(self, len(start) - 1, window)
        try:
            if state.n_out != len(start) - 1:
                raise ValueError(f"the map has {len(start) - 1} outputs, the state {state.n_out}")
            streams, ptrs, sizes = _stream_arrays(streams, named=set(int(f) for f in np.unique(frame)))
            row0, col0 = state.window[:2]
            if self.lib.ebcc_hip_project_shard(self.ctx, ptrs, sizes, n, row0, col0, ctypes.byref(state.map(start, frame, weight))):
                self._fail("ebcc_hip_project_shard")
            return state.result() if own else state
        finally:
            if own:
                state.close()

    def series(self, streams, regions, w_row=None, w_pix=None, threshold=None):
        """Statistics over regions at every time step straight from the streams (ebcc_hip_series_shard): `regions` is an int
        array (R, 4) of (row0, col0, rows, cols) - boxes of the frame, which may overlap and repeat -, w_row (H,) float64 a
        weight per row (lat_weights), w_pix (H, W) float32 a weight per pixel, 0 where a pixel is masked out; both default to
        1 and must be finite and not negative.  Only the bounding box of the regions is decoded, and no decoded frame leaves
        the device -> a SeriesResult with one record per stream and region.  w_pix is uploaded once for the call.  ValueError
        for arguments the engine would refuse, RuntimeError for what the call reports, such as a malformed stream."""
        area = _Area(self, regions, w_row, w_pix, threshold)
        try:
            return SeriesResult(area.run(streams), area.weight())
        finally:
            area.close()

    def regrid(self, streams, row_map, col_map, out=None):
        """The same fields on another grid straight from the streams (ebcc_hip_regrid_host_frames): row_map and col_map are
        regrid.AxisMap objects - identity_map, flip_map, block_mean_map, conservative_map, linear_map or hand-made - and every
        frame is resampled on the device by the rule include/ebcc_hip.h states -> (n, row_map.n_out, col_map.n_out) float32.
        Only the bounding box of the supports is decoded and only the resampled frames cross PCIe.  `out`: a C-contiguous
        float32 array to fill, or an integer - a 4-byte aligned device pointer with room for the result, which is then
        written there (ebcc_hip_regrid_shard) and returned as given.  ValueError for a map the engine refuses (checked here,
        before the call), RuntimeError for what the call reports, such as a malformed stream."""
        n = len(streams)
        if n < 1:
            raise ValueError("no streams")
        spec = _regrid.regrid_spec(row_map, col_map)
        if self.lib.ebcc_hip_regrid_check(self.h, self.w, ctypes.byref(spec), None) < 0:
            raise ValueError((self.lib.ebcc_hip_last_error() or b"?").decode())
        streams, ptrs, sizes = _stream_arrays(streams)
        if isinstance(out, (int, np.integer)):
            if self.lib.ebcc_hip_regrid_shard(self.ctx, ptrs, sizes, n, ctypes.byref(spec), int(out)):
                self._fail("ebcc_hip_regrid_shard")
            return out
        shape = (n, row_map.n_out, col_map.n_out)
        if out is None:
            out = np.empty(shape, np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == n * shape[1] * shape[2]
        if self.lib.ebcc_hip_regrid_host_frames(self.ctx, ptrs, sizes, n, ctypes.byref(spec), out.ctypes.data):
            self._fail("ebcc_hip_regrid_host_frames")
        return out

    def encode_groups(self, groups, hard=False, max_rounds=0):
        """Many variables in one device call: `groups` is a list of (frames, base_cr, residual_opt[, range_of_group]) - frames
        (n, H, W) float32 in host memory (each group its own array, any n), base_cr and residual_opt as for frame_config,
        range_of_group=True: a relative error target counts against (max - min) over the whole group, as
        ebcc_encode_chunking_compat restates it.  -> one list of EBCC frame streams (bytes) per group; every stream is what
        encode() gives for that frame with the group's config.  All frames run as one list, in batches on the two engine sets.
        hard=True: as in encode(); the result is then (lists of streams, report) with one BOUND_REPORT record per frame, all
        groups in order."""
        if not groups:
            raise ValueError("no groups")
        arrays, table = [], (FrameGroup * len(groups))()
        for g, item in enumerate(groups):
            frames, base_cr, residual_opt = item[:3]
            a = np.ascontiguousarray(frames, np.float32)
            if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (self.h, self.w):
                raise ValueError(f"group {g}: frames must be (n, {self.h}, {self.w}) with n >= 1, got {a.shape}")
            arrays.append(a)                                            # (kept alive for the call)
            table[g].frames, table[g].n_frames = a.ctypes.data, a.shape[0]
            table[g].config = frame_config(self.h, self.w, base_cr, residual_opt)
            table[g].range_of_group = int(bool(item[3])) if len(item) > 3 else 0
        total = sum(a.shape[0] for a in arrays)
        outs = (ctypes.c_void_p * total)()
        sizes = (ctypes.c_size_t * total)()
        report = np.zeros(total, BOUND_REPORT)
        if hard:
            if self.lib.ebcc_hip_encode_host_frames_groups_hard(self.ctx, table, len(groups), int(max_rounds), outs, sizes,
                                                                report.ctypes.data) not in (0, 3):
                self._fail("ebcc_hip_encode_host_frames_groups_hard")
        elif self.lib.ebcc_hip_encode_host_frames_groups(self.ctx, table, len(groups), outs, sizes):
            self._fail("ebcc_hip_encode_host_frames_groups")
        res, at = [], 0
        for a in arrays:
            res.append([ctypes.string_at(outs[i], sizes[i]) for i in range(at, at + a.shape[0])])
            at += a.shape[0]
        for i in range(total):
            self.lib.free_buffer(outs[i])
        return (res, report) if hard else res

    def decode(self, streams, out=None, window=None):
        """list of EBCC frame streams (bytes), any number -> (n, H, W) float32; `out`: a C-contiguous float32 array to decode
        into (the frames cross PCIe straight into it; its pages are mapped while the GPU decodes, one batch is downloaded
        beside the kernels of the next).  `window` = (row0, col0, rows, cols): only that box of every frame, (n, rows, cols) -
        bit for bit the crop of the full decode, from the code-blocks the box depends on; nothing else is decoded or
        downloaded."""
        n = len(streams)
        assert n >= 1
        streams, ptrs, sizes = _stream_arrays(streams)
        if window is not None:
            row0, col0, rows, cols = (int(v) for v in window)
            if min(row0, col0) < 0 or rows < 1 or cols < 1 or row0 + rows > self.h or col0 + cols > self.w:
                raise ValueError(f"window {tuple(window)} is empty or not inside the {self.h} x {self.w} frame")
            if out is None:
                out = np.empty((n, rows, cols), np.float32)
            assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == n * rows * cols
            if self.lib.ebcc_hip_decode_host_frames_window(self.ctx, ptrs, sizes, n, row0, col0, rows, cols, out.ctypes.data):
                self._fail("ebcc_hip_decode_host_frames_window")
            return out
        if out is None:
            out = np.empty((n, self.h, self.w), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == n * self.h * self.w
        t0 = time.perf_counter()
        if self.lib.ebcc_hip_decode_host_frames(self.ctx, ptrs, sizes, n, out.ctypes.data):
            self._fail("ebcc_hip_decode_host_frames")
        if os.environ.get("EBCC_H5_TIMING"):
            print(f"h5_batch.decode: {n} frames decoded and downloaded in {1e3 * (time.perf_counter() - t0):.1f} ms", file=sys.stderr, flush=True)
        return out

    def decode_boxes(self, streams, boxes, rows, cols, out=None):
        """Any boxes of any frames: `boxes` is an int array (k, 3) of (frame, row0, col0) in non-decreasing order of frame,
        every box rows x cols -> (k, rows, cols) float32, box e bit for bit streams[frame_e] decoded and cropped to
        [row0, row0 + rows) x [col0, col0 + cols).  A frame is decoded once, from the code-blocks its boxes depend on; a
        frame no box names is not read (its entry of `streams` may be None).  Repeated and overlapping boxes are fine and k
        is not limited by the engine's capacity.  ValueError for a list the engine refuses (checked here, before the call);
        RuntimeError for what the call itself reports, such as a malformed stream."""
        n = len(streams)
        rows, cols = int(rows), int(cols)
        b = _box_array(boxes)
        if rows < 1 or cols < 1 or rows > self.h or cols > self.w:
            raise ValueError(f"boxes of {rows} x {cols} are empty or not inside the {self.h} x {self.w} frame")
        if b.min() < 0 or (b[:, 0] >= n).any():
            raise ValueError(f"a box names a frame outside the {n} streams, or has a negative origin")
        if (b[:, 1] > self.h - rows).any() or (b[:, 2] > self.w - cols).any():
            raise ValueError(f"a box of {rows} x {cols} is not inside the {self.h} x {self.w} frame")
        if (np.diff(b[:, 0]) < 0).any():
            raise ValueError("boxes must be in non-decreasing order of their frames")
        k = len(b)
        streams, ptrs, sizes = _stream_arrays(streams, named=set(int(f) for f in np.unique(b[:, 0])))
        table = np.ascontiguousarray(b, np.uint64)                       # == ebcc_hip_box[k]
        if out is None:
            out = np.empty((k, rows, cols), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == k * rows * cols
        if self.lib.ebcc_hip_decode_host_frames_boxes(self.ctx, ptrs, sizes, n, table.ctypes.data, k, rows, cols, out.ctypes.data):
            self._fail("ebcc_hip_decode_host_frames_boxes")
        return out

    def decode_placed(self, streams, boxes, out):
        """Boxes of their own sizes, each put into its own rectangle of `out`: `boxes` is an int array (k, 7) of (frame, row0,
        col0, rows, cols, out_offset, out_pitch) in non-decreasing order of frame; sample (y, x) of box e - streams[frame_e]
        decoded and cropped to [row0, row0 + rows) x [col0, col0 + cols), bit for bit - goes to out.ravel()[out_offset +
        y * out_pitch + x].  `out` is a C-contiguous float32 array; only the rectangles are written, everything else of it keeps
        its values (where rectangles overlap the samples are unspecified).  Otherwise as decode_boxes; returns `out`."""
        n = len(streams)
        b = np.asarray(boxes)
        if b.ndim != 2 or b.shape[1] != 7 or b.shape[0] < 1 or b.dtype.kind not in "iu":
            raise ValueError("boxes must be a non-empty integer array of shape (k, 7): frame, row0, col0, rows, cols, out_offset, out_pitch")
        b = b.astype(np.int64)
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("out must be a writable C-contiguous float32 array")
        frame, row0, col0, rows, cols, at, pitch = b.T
        if b.min() < 0 or (frame >= n).any():
            raise ValueError(f"a box names a frame outside the {n} streams, or has a negative field")
        if (rows < 1).any() or (cols < 1).any() or (rows > self.h).any() or (cols > self.w).any() or (row0 > self.h - rows).any() or (col0 > self.w - cols).any():
            raise ValueError(f"a box is empty or not inside the {self.h} x {self.w} frame")
        if (pitch < cols).any():
            raise ValueError("a box's pitch is smaller than its rows")
        if (at + (rows - 1) * pitch + cols > out.size).any():
            raise ValueError(f"a box does not end inside the {out.size} floats of out")
        if (np.diff(frame) < 0).any():
            raise ValueError("boxes must be in non-decreasing order of their frames")
        streams, ptrs, sizes = _stream_arrays(streams, named=set(int(f) for f in np.unique(frame)))
        table = np.ascontiguousarray(b, np.uint64)                       # == ebcc_hip_placed_box[k]
        if self.lib.ebcc_hip_decode_host_frames_placed(self.ctx, ptrs, sizes, n, table.ctypes.data, len(b), out.ctypes.data, out.size):
            self._fail("ebcc_hip_decode_host_frames_placed")
        return out


_SUPER = 16         # batches handed to the engine per call by write_frames / read_frames (filling and draining the two sets costs ~half a batch)

# Engines are expensive to make (tens of GB of device workspace for 256 frames of 721 x 1440) and cheap to keep: the
# helpers below share ONE per (height, width, device) for the life of the process - a codec made for more frames serves a
# request for fewer, a larger request replaces it (the old one is closed first), and when the device has no room for a new
# engine every cached one is closed and the creation is tried once more.  close_cached() gives the memory back; callers
# that hold datasets of many geometries in one process and want the memory between them call it themselves.
#
# Threads may share the cache.  One lock guards it, and a codec made while it is held, so two threads that ask for a missing
# geometry at once get one engine.  The helpers of this module hold their codec for as long as they are inside it
# (held_codec); a replacement and close_cached() wait for the last holder before they close an engine, so no call loses its
# engine under it.  A codec taken with cached_codec() alone is not held: whoever keeps one across calls of other threads
# that may replace or close it uses held_codec.  A holder that asks for a larger codec of its own geometry, or calls
# close_cached(), from inside its `with` block would wait for itself.
_codecs = {}
_cache = threading.Condition()                                  # guards _codecs and _holders; notified when a holder leaves
_holders = {}                                                   # codec -> the number of held_codec blocks that are inside it


def _close_idle(c):
    """close `c` once nobody holds it (the cache's lock held; it is released while waiting)"""
    while _holders.get(c):
        _cache.wait()
    c.close()


def _cached(height, width, max_frames, device, hold):
    key, max_frames = (int(height), int(width), int(device)), int(max_frames)
    with _cache:
        while True:
            c = _codecs.get(key)
            if c is not None and c.ctx and c.max_frames >= max_frames:
                break
            if c is not None:
                _close_idle(c)
                if _codecs.get(key) is c:
                    del _codecs[key]
                continue                                        # (another thread may have made the larger one meanwhile)
            try:
                c = BatchCodec(height, width, max_frames, device)
            except RuntimeError:
                _close_all()                                    # (other geometries' engines may hold the memory)
                if key in _codecs:
                    continue
                c = BatchCodec(height, width, max_frames, device)
            _codecs[key] = c
            break
        if hold:
            _holders[c] = _holders.get(c, 0) + 1
        return c


def _release(c):
    with _cache:
        _holders[c] -= 1
        if not _holders[c]:
            del _holders[c]
        _cache.notify_all()


def cached_codec(height, width, max_frames=256, device=0):
    return _cached(height, width, max_frames, device, hold=False)


@contextlib.contextmanager
def held_codec(height, width, max_frames=256, device=0, codec=None):
    """The cached codec of a geometry, held for the `with` block: no other thread's larger request and no close_cached()
    closes it before the block is left.  `codec`: a codec of the caller's own, handed through as it is."""
    if codec is not None:
        yield codec
        return
    c = _cached(height, width, max_frames, device, hold=True)
    try:
        yield c
    finally:
        _release(c)


def _close_all():
    for key, c in list(_codecs.items()):
        _close_idle(c)
        if _codecs.get(key) is c:
            del _codecs[key]


def close_cached():
    with _cache:
        _close_all()


import atexit  # noqa: E402

atexit.register(close_cached)


def create_dataset(group, name, shape, base_cr, residual_opt=("none", None), **kw):
    """An EBCC-filtered float32 dataset of shape (..., H, W) with one frame per chunk."""
    h, w = shape[-2:]
    return group.create_dataset(name, shape=shape,
                                **EBCC_Filter(base_cr=base_cr, height=h, width=w, residual_opt=residual_opt, data_dim=len(shape)), **kw)


def _not_met(report, what):
    missed = int((report["met"] == 0).sum())
    if missed:
        raise BoundNotMet(f"{what}: {missed} of {len(report)} frames stay over their bound "
                          f"(worst {float((report['achieved'] / report['target']).max()):.4f} of it); nothing of this call was written", report)


def write_frames(dset, data, base_cr, residual_opt=("none", None), batch=256, codec=None, hard=False, max_rounds=0):
    """Code `data` (same shape as `dset`, frames in its last two axes) in device batches and store every frame
    as a pre-filtered chunk.  `base_cr` / `residual_opt` must be the dataset's filter parameters.  hard=True: the chunks hold
    their bound for every reader (BatchCodec.encode(hard=True)); returns the BOUND_REPORT array, shaped as the leading axes,
    and raises BoundNotMet - before the frames of that device call are stored - when a frame stays over its bound."""
    data = np.asarray(data, np.float32)
    assert tuple(data.shape) == tuple(dset.shape) and dset.chunks == (1,) * (data.ndim - 2) + data.shape[-2:]
    h, w = data.shape[-2:]
    flat = data.reshape((-1, h, w))
    lead = data.shape[:-2]
    cfg = frame_config(h, w, base_cr, residual_opt)
    reports = []
    with held_codec(h, w, min(batch, len(flat)), codec=codec) as codec:
        step = _SUPER * codec.max_frames                        # (several batches per call: they alternate between two engine sets)
        for lo in range(0, len(flat), step):
            if hard:
                streams, report = codec.encode(flat[lo:lo + step], cfg, hard=True, max_rounds=max_rounds)
                _not_met(report, f"{dset.name}, frames {lo}..{lo + len(report) - 1}")
                reports.append(report)
            else:
                streams = codec.encode(flat[lo:lo + step], cfg)
            for i, s in enumerate(streams):
                idx = np.unravel_index(lo + i, lead) if lead else ()
                dset.id.write_direct_chunk(tuple(int(v) for v in idx) + (0, 0), s, filter_mask=0)
    return np.concatenate(reports).reshape(tuple(lead)) if hard else None


def filter_options(dset):
    """(base_cr, residual_opt) of an EBCC-filtered dataset, from the cd_values of its filter 308 as
    /root/reference/src/h5z_ebcc.c:38-93 reads them: (height, width, f32 bits of base_cr, mode[, f32 bits of the error])."""
    plist = dset.id.get_create_plist()
    for i in range(plist.get_nfilters()):
        code, _flags, cd, _name = plist.get_filter(i)
        if code == EBCC_Filter.FILTER_ID:
            if len(cd) < 4 or (cd[3] and len(cd) < 5) or (int(cd[0]), int(cd[1])) != tuple(dset.shape[-2:]):
                raise ValueError(f"{dset.name}: filter 308 parameters {tuple(cd)} do not describe frames of {dset.shape[-2:]}")
            bits = lambda v: float(np.array([v], np.uint32).view(np.float32)[0])  # noqa: E731
            mode = {0: "none", 1: "max_error_target", 2: "relative_error_target"}.get(int(cd[3]))
            if mode is None:
                raise ValueError(f"{dset.name}: unknown residual mode {cd[3]}")
            return bits(cd[2]), (mode, bits(cd[4]) if cd[3] else None)
    raise ValueError(f"{dset.name}: not an EBCC-filtered dataset")


def write_variables(items, batch=256, codec=None, hard=False, max_rounds=0):
    """Several variables in one device call: `items` is a list of (dset, first_frame, frames) over one-frame-per-chunk
    EBCC-filtered datasets of one frame geometry - frames (n, H, W) float32 go to the chunks first_frame .. first_frame + n - 1
    of dset, counted in C order over its leading axes.  Every dataset's own filter-308 parameters are its group's config
    (filter_options), all groups are coded by one BatchCodec.encode_groups call, then every chunk is stored pre-filtered.
    The chunk bytes are those write_frames gives dataset by dataset.  hard=True: as in write_frames; returns one BOUND_REPORT
    array per item and raises BoundNotMet, with nothing stored, when a frame stays over its bound."""
    if not items:
        raise ValueError("no items")
    h, w = items[0][0].shape[-2:]
    groups, total = [], 0
    for dset, first, frames in items:
        frames = np.ascontiguousarray(frames, np.float32)
        lead = dset.shape[:-2]
        n = int(np.prod(lead)) if lead else 1
        if tuple(dset.shape[-2:]) != (h, w) or dset.chunks != (1,) * len(lead) + (h, w):
            raise ValueError(f"{dset.name}: one-frame chunks of {h} x {w} are needed, got chunks {dset.chunks}")
        if frames.ndim != 3 or frames.shape[1:] != (h, w) or first < 0 or first + len(frames) > n or len(frames) < 1:
            raise ValueError(f"{dset.name}: frames {frames.shape} from frame {first} on do not fit the dataset's {n} frames")
        base_cr, opt = filter_options(dset)
        groups.append((frames, base_cr, opt))
        total += len(frames)
    report = None
    with held_codec(h, w, min(batch, total), codec=codec) as codec:
        if hard:
            coded, report = codec.encode_groups(groups, hard=True, max_rounds=max_rounds)
            _not_met(report, "write_variables")
        else:
            coded = codec.encode_groups(groups)
    for (dset, first, _), streams in zip(items, coded):
        lead = dset.shape[:-2]
        for i, s in enumerate(streams):
            idx = np.unravel_index(first + i, lead) if lead else ()
            dset.id.write_direct_chunk(tuple(int(v) for v in idx) + (0, 0), s, filter_mask=0)
    if hard:
        cuts = np.cumsum([len(g[0]) for g in groups])[:-1]
        return np.split(report, cuts)


def audit_dataset(dset, data, batch=256, codec=None):
    """The error of an EBCC-filtered one-frame-per-chunk dataset against `data` (same shape), measured on the device: the raw
    chunks are fetched as read_frames fetches them and audited (BatchCodec.audit) against the dataset's own filter bound - the
    error of a max_error_target, error * (max - min) of the frame for a relative_error_target in float32 as the encoder
    multiplies it, none for a dataset without a residual layer -> a FRAME_ERROR array shaped as the leading axes; a frame
    holds its bound where n_over == 0."""
    data = np.asarray(data, np.float32)
    if tuple(data.shape) != tuple(dset.shape):
        raise ValueError(f"{dset.name}: data of shape {data.shape} against a dataset of {dset.shape}")
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    flat = data.reshape((-1, h, w))
    n = len(flat)
    _base_cr, (mode, err) = filter_options(dset)
    out = np.zeros(n, FRAME_ERROR)
    with held_codec(h, w, min(batch, n), codec=codec) as codec:
        step = _SUPER * codec.max_frames
        for lo in range(0, n, step):
            part = flat[lo:lo + step]
            bound = None
            if mode == "max_error_target":
                bound = np.float32(err)
            elif mode == "relative_error_target":
                bound = np.float32(err) * (part.max(axis=(1, 2)) - part.min(axis=(1, 2))).astype(np.float32)
            out[lo:lo + len(part)] = codec.audit(_read_chunks(dset, range(lo, lo + len(part))), part, bound)
    return out.reshape(tuple(lead))


def _box(sl, n, what):
    """(first, count) of a slice over an axis of n samples (None: all of it); step 1 and not empty"""
    if sl is None:
        return 0, n
    if not isinstance(sl, slice):
        raise TypeError(f"{what} must be a slice or None")
    first, stop, step = sl.indices(n)
    if step != 1 or stop <= first:
        raise ValueError(f"{what}: a non-empty slice of step 1 is needed, got {sl}")
    return first, stop - first


def read_frames(dset, batch=256, codec=None, rows=None, cols=None):
    """Read an EBCC-filtered one-frame-per-chunk dataset by decoding its raw chunks in device batches, several batches per
    call (they alternate between two engine sets: one is downloaded while the next decodes).  The raw chunks of the next
    call are fetched from the file (h5py, one call per chunk) on a helper thread meanwhile; the frames land straight in
    their place in the result.  `rows` / `cols`: slices (step 1) over the frames' two axes - only that box of every frame is
    decoded and downloaded, and the result has the shape lead + (rows, cols); it equals read_frames(dset)[..., rows, cols]."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    (row0, nrows), (col0, ncols) = _box(rows, h, "rows"), _box(cols, w, "cols")
    window = None if (nrows, ncols) == (h, w) else (row0, col0, nrows, ncols)
    out = np.empty((n, nrows, ncols), np.float32)
    with held_codec(h, w, min(batch, n), codec=codec) as codec:
        step = _SUPER * codec.max_frames

        def read(lo):
            t0 = time.perf_counter()
            try:
                return _read_chunks(dset, range(lo, min(n, lo + step)))
            finally:
                if lo == 0 and os.environ.get("EBCC_H5_TIMING"):
                    print(f"h5_batch.read_frames: first {min(n, step)} chunks fetched in {1e3 * (time.perf_counter() - t0):.1f} ms", file=sys.stderr, flush=True)

        def work(lo, raw):
            codec.decode(raw, out=out[lo:lo + len(raw)], window=window)

        _prefetched(read, n, step, work)
    return out.reshape(tuple(lead) + (nrows, ncols))


def _lead_bins(lead, bins, n_bins, noun):
    """`bins` of a dataset with the leading axes `lead` (None: everything in bin 0, -1: skipped) -> (b, named, n_bins): the
    bins in C order as int64, the indices of those that are named, and n_bins (None: the largest bin + 1).  noun: "frame" /
    "step", for the messages."""
    n = int(np.prod(lead)) if lead else 1
    b = np.zeros(n, np.int64) if bins is None else np.asarray(bins)
    if b.dtype.kind not in "iu" or b.size != n or (bins is not None and tuple(b.shape) != tuple(lead)):
        raise ValueError(f"bins must be an integer array of shape {tuple(lead)}")
    b = b.astype(np.int64).reshape(-1)
    named = np.nonzero(b >= 0)[0]
    if len(named) < 1 or b.min() < -1:
        raise ValueError(f"bins must name at least one {noun}, and -1 is the only negative value")
    n_bins = int(b.max()) + 1 if n_bins is None else int(n_bins)
    if b.max() >= n_bins:
        raise ValueError(f"a {noun} names bin {int(b.max())} of {n_bins}")
    return b, named, n_bins


def _prefetched(read, n, step, work):
    """work(lo, read(lo)) for lo = 0, step, .. below n, one after the other: while a call works, the next one's chunks are read
    on a helper thread, which is joined before the call returns; a failure of a read is raised on the caller's thread."""
    def fetch(lo, box):
        try:
            box.append(read(lo))
        except BaseException as e:                                  # (handed to the caller's thread)
            box.append(e)

    box = []
    fetch(0, box)
    for lo in range(0, n, step):
        raw = box[0]
        if isinstance(raw, BaseException):
            raise raw
        box, t = [], None
        if lo + step < n:
            t = threading.Thread(target=fetch, args=(lo + step, box))
            t.start()
        try:
            work(lo, raw)
        finally:
            if t:
                t.join()


def reduce_frames(dset, bins=None, n_bins=None, rows=None, cols=None, threshold=None, batch=256, codec=None):
    """Statistics over time of an EBCC-filtered one-frame-per-chunk dataset, folded on the device (BatchCodec.reduce): `bins`
    is an integer array shaped like the leading axes - the bin of every frame, -1: skip the frame (its chunk is not fetched);
    None: everything in one bin -, n_bins defaults to bins.max() + 1, `rows` / `cols` are slices (step 1) as in read_frames.
    -> a ReduceResult whose every statistic equals the same reduction - a loop over the frames in C order of the leading axes,
    in float64 - of read_frames(dset)[..., rows, cols]; no frame is downloaded.  The chunks are fetched as read_frames fetches
    them, the next call's on a helper thread, and folded call after call into one device-resident state, so the dataset need
    not fit into host memory."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    (row0, nrows), (col0, ncols) = _box(rows, h, "rows"), _box(cols, w, "cols")
    b, named, n_bins = _lead_bins(lead, bins, n_bins, "frame")
    with contextlib.ExitStack() as stack:
        codec = stack.enter_context(held_codec(h, w, min(batch, len(named)), codec=codec))
        step = _SUPER * codec.max_frames
        state = stack.enter_context(codec.reduce_state(n_bins, (row0, col0, nrows, ncols), threshold))

        def work(lo, raw):
            codec.reduce(raw, bins=b[named[lo:lo + step]], state=state)

        _prefetched(lambda lo: _read_chunks(dset, named[lo:lo + step]), len(named), step, work)
        return state.result()


def pair_frames(dset_x, dset_y, bins=None, n_bins=None, rows=None, cols=None, threshold=None, magnitude=True, batch=256, codec=None):
    """Co-moments and vector magnitude over time of two EBCC-filtered one-frame-per-chunk datasets of the same shape, folded on
    the device (BatchCodec.pair): frame f of dset_x is paired with frame f of dset_y - u10 and v10, or a variable and itself
    shifted.  `bins`, n_bins, `rows` / `cols` as in reduce_frames (-1: the step is skipped, its chunks are not fetched);
    `threshold`: count the steps whose magnitude is above it; magnitude=False: co-moments only.  -> a PairResult whose every
    array equals the same loop, step after step in C order of the leading axes, over read_frames of both datasets; no frame is
    downloaded.  The chunks of both are fetched as reduce_frames fetches them, the next call's on a helper thread, and folded
    call after call into one device-resident state.  ValueError for datasets of different shape."""
    if tuple(dset_x.shape) != tuple(dset_y.shape):
        raise ValueError(f"the datasets have the shapes {tuple(dset_x.shape)} and {tuple(dset_y.shape)}")
    h, w = dset_x.shape[-2:]
    lead = dset_x.shape[:-2]
    (row0, nrows), (col0, ncols) = _box(rows, h, "rows"), _box(cols, w, "cols")
    b, named, n_bins = _lead_bins(lead, bins, n_bins, "step")
    with contextlib.ExitStack() as stack:
        codec = stack.enter_context(held_codec(h, w, max(2, min(batch, 2 * len(named))), codec=codec))
        step = _SUPER * max(1, codec.max_frames // 2)                   # (steps a call: two frames each)
        state = stack.enter_context(codec.pair_state(n_bins, (row0, col0, nrows, ncols), threshold, magnitude))

        def work(lo, raw):
            codec.pair(raw[0], raw[1], bins=b[named[lo:lo + step]], state=state)

        _prefetched(lambda lo: (_read_chunks(dset_x, named[lo:lo + step]), _read_chunks(dset_y, named[lo:lo + step])), len(named), step, work)
        return state.result()


def spell_frames(dset, threshold, below=False, min_len=1, bins=None, when=None, fresh=None, n_bins=None, rows=None, cols=None,
                 what=("runs", "events", "extremes"), batch=256, codec=None):
    """Run lengths and event timing over time of an EBCC-filtered one-frame-per-chunk dataset, folded on the device
    (BatchCodec.spells): every frame is a step, in C order of the leading axes.  `bins`, n_bins, `rows` / `cols` as in
    reduce_frames (-1: the step is skipped, its chunk is not fetched); `when` and `fresh` are arrays shaped like the leading
    axes - the label of every step (None: its index in C order) and the flag that begins a new visit to its bin -; threshold,
    below, min_len and what as in BatchCodec.spells.  -> a SpellResult whose every array equals the same loop, step after step,
    over read_frames(dset)[..., rows, cols]; no frame is downloaded.  The chunks are fetched as reduce_frames fetches them, the
    next call's on a helper thread, and folded call after call into one device-resident state, which carries the open runs."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    (row0, nrows), (col0, ncols) = _box(rows, h, "rows"), _box(cols, w, "cols")
    b, named, n_bins = _lead_bins(lead, bins, n_bins, "step")
    labels = np.arange(n, dtype=np.int64) if when is None else np.asarray(when)
    if labels.dtype.kind not in "iu" or labels.size != n or (when is not None and tuple(labels.shape) != tuple(lead)):
        raise ValueError(f"when must be an integer array of shape {tuple(lead)}")
    labels = labels.astype(np.int64).reshape(-1)
    flags = np.zeros(n, bool) if fresh is None else np.asarray(fresh).astype(bool)
    if flags.size != n or (fresh is not None and tuple(flags.shape) != tuple(lead)):
        raise ValueError(f"fresh must be an array of shape {tuple(lead)}")
    flags = flags.reshape(-1)
    with contextlib.ExitStack() as stack:
        codec = stack.enter_context(held_codec(h, w, min(batch, len(named)), codec=codec))
        step = _SUPER * codec.max_frames
        state = stack.enter_context(codec.spell_state(threshold, below, min_len, n_bins, (row0, col0, nrows, ncols), what))

        def work(lo, raw):
            part = named[lo:lo + step]
            codec.spells(raw, None, bins=b[part], when=labels[part], fresh=flags[part], state=state)

        _prefetched(lambda lo: _read_chunks(dset, named[lo:lo + step]), len(named), step, work)
        return state.result()


def quantile_frames(dset, q, bins=None, n_bins=None, rows=None, cols=None, method="linear", batch=256, codec=None):
    """Quantiles over time of an EBCC-filtered one-frame-per-chunk dataset, selected on the device (BatchCodec.quantiles): `q`
    a number or a sequence of numbers in [0, 1], `bins`, n_bins, `rows` / `cols` as in reduce_frames (a month per frame gives
    a percentile climatology), `method` as in BatchCodec.quantiles -> a QuantileResult whose values (n_bins, len(q), rows,
    cols) are those quantiles of read_frames(dset)[..., rows, cols] over the frames of each bin; no frame is downloaded.  The
    chunks of the named frames are fetched once - the eight passes of the select run over the streams in host memory, which
    therefore must hold them (not the decoded frames)."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    (row0, nrows), (col0, ncols) = _box(rows, h, "rows"), _box(cols, w, "cols")
    b, named, n_bins = _lead_bins(lead, bins, n_bins, "frame")
    with held_codec(h, w, min(batch, len(named)), codec=codec) as codec:
        raw = _read_chunks(dset, named)
        return codec.quantiles(raw, q, bins=b[named], n_bins=n_bins, window=(row0, col0, nrows, ncols), method=method)


def project_frames(dset, weights, rows=None, cols=None, batch=256, codec=None):
    """Weighted sums over time of an EBCC-filtered one-frame-per-chunk dataset, folded on the device (BatchCodec.project):
    `weights` is a time map over the frames counted in C order of the leading axes - a dense [n_out][n_frames] array or a
    (start, frame, weight) triple (time_map_terms; trend_weights and running_mean_weights make two) -, `rows` / `cols` are
    slices (step 1) as in read_frames -> a ProjectResult whose values equal, for every output, a loop over its terms in
    increasing frame, acc = acc + weight * float64(x), on read_frames(dset)[..., rows, cols]; no frame is downloaded.  Only the
    chunks of frames that some term names are fetched, as read_frames fetches them, the next call's on a helper thread, and
    folded call after call into one device-resident state, so the dataset need not fit into host memory."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    (row0, nrows), (col0, ncols) = _box(rows, h, "rows"), _box(cols, w, "cols")
    terms = time_map_terms(weights, n_frames=n)
    named = np.unique(terms[1]).astype(np.int64)
    with contextlib.ExitStack() as stack:
        codec = stack.enter_context(held_codec(h, w, min(batch, len(named)), codec=codec))
        step = _SUPER * codec.max_frames
        state = stack.enter_context(codec.map_state(len(terms[0]) - 1, (row0, col0, nrows, ncols)))

        def work(lo, raw):
            # the call's streams are the named frames of this step alone: its terms, with their frames counted among them
            start, frame, weight = _terms_of_range(terms, int(named[lo]), int(named[lo:lo + step][-1]) + 1)
            at = np.searchsorted(named[lo:lo + step], frame.astype(np.int64) + int(named[lo])).astype(np.uint32)
            codec.project(raw, (start, at, weight), state=state)

        _prefetched(lambda lo: _read_chunks(dset, named[lo:lo + step]), len(named), step, work)
        return state.result()


def series_frames(dset, regions, frames=None, w_row=None, w_pix=None, threshold=None, batch=256, codec=None):
    """Statistics over regions at every time step of an EBCC-filtered one-frame-per-chunk dataset, folded on the device
    (BatchCodec.series): `frames` names the frames - counted in C order over the leading axes, in any order; None: all of them
    -, regions, w_row, w_pix and threshold are those of BatchCodec.series -> a SeriesResult with one record per named frame, in
    their order, and region; every statistic equals the fold of include/ebcc_hip.h over read_frames(dset) at those frames.  No
    frame is downloaded.  The chunks are fetched as read_frames fetches them, the next call's on a helper thread, w_pix is
    uploaded once, and the records of the calls are concatenated, so the dataset need not fit into host memory."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    named = np.arange(n) if frames is None else np.asarray(frames)
    if named.ndim != 1 or len(named) < 1 or named.dtype.kind not in "iu" or named.min() < 0 or named.max() >= n:
        raise ValueError(f"frames must be a non-empty list of integers in [0, {n})")
    with contextlib.ExitStack() as stack:
        codec = stack.enter_context(held_codec(h, w, min(batch, len(named)), codec=codec))
        step = _SUPER * codec.max_frames
        area = _Area(codec, regions, w_row, w_pix, threshold)
        stack.callback(area.close)
        parts = []

        def work(lo, raw):
            parts.append(area.run(raw))

        _prefetched(lambda lo: _read_chunks(dset, named[lo:lo + step]), len(named), step, work)
        return SeriesResult(np.concatenate(parts), area.weight())


def read_regridded(dset, row_map, col_map, frames=None, batch=256, codec=None):
    """The frames of an EBCC-filtered one-frame-per-chunk dataset on another grid (BatchCodec.regrid): `frames` names the frames
    - counted in C order over the leading axes, in any order; None: all of them -, row_map and col_map are regrid.AxisMap
    objects -> (len(frames), row_map.n_out, col_map.n_out) float32, frame k equal to the rule of include/ebcc_hip.h applied to
    read_frames(dset) at frame k.  No decoded frame is downloaded.  The chunks are fetched as series_frames fetches them, the
    next call's on a helper thread."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    named = np.arange(n) if frames is None else np.asarray(frames)
    if named.ndim != 1 or len(named) < 1 or named.dtype.kind not in "iu" or named.min() < 0 or named.max() >= n:
        raise ValueError(f"frames must be a non-empty list of integers in [0, {n})")
    with contextlib.ExitStack() as stack:
        codec = stack.enter_context(held_codec(h, w, min(batch, len(named)), codec=codec))
        step = _SUPER * codec.max_frames
        out = np.empty((len(named), row_map.n_out, col_map.n_out), np.float32)

        def work(lo, raw):
            codec.regrid(raw, row_map, col_map, out=out[lo:lo + len(raw)])

        _prefetched(lambda lo: _read_chunks(dset, named[lo:lo + step]), len(named), step, work)
        return out


def read_boxes(dset, boxes, rows, cols, batch=256, codec=None):
    """Boxes of rows x cols out of an EBCC-filtered one-frame-per-chunk dataset: `boxes` is an int array (k, 3) of
    (frame, row0, col0), the frame counted in C order over the leading axes, in any order -> (k, rows, cols), box e equal to
    read_frames(dset).reshape(-1, H, W)[frame_e, row0:row0 + rows, col0:col0 + cols].  Only the chunks of the frames the boxes
    name are fetched from the file, and each of them is decoded once (BatchCodec.decode_boxes)."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    b = _box_array(boxes)
    if b[:, 0].min() < 0 or b[:, 0].max() >= n:
        raise ValueError(f"a box names a frame outside the {n} frames of the dataset")
    order = np.argsort(b[:, 0], kind="stable")
    b = b[order]
    frames = np.unique(b[:, 0])                                         # (sorted)
    out = np.empty((len(b), int(rows), int(cols)), np.float32)
    with held_codec(h, w, min(batch, len(frames)), codec=codec) as codec:
        step = _SUPER * codec.max_frames
        for lo in range(0, len(frames), step):
            part = frames[lo:lo + step]
            raw = _read_chunks(dset, part)
            e0, e1 = np.searchsorted(b[:, 0], part[0], "left"), np.searchsorted(b[:, 0], part[-1], "right")
            local = b[e0:e1].copy()
            local[:, 0] = np.searchsorted(part, local[:, 0])
            codec.decode_boxes(raw, local, rows, cols, out=out[e0:e1])
    res = np.empty_like(out)
    res[order] = out
    return res


def read_points(dset, rows_idx, cols_idx, batch=256, codec=None):
    """The series of K samples through every frame - stations - as lead + (K,): read_frames(dset)[..., rows_idx, cols_idx] for
    two integer sequences of length K, from 1 x 1 boxes (read_boxes): every frame is decoded once, from the few code-blocks
    its K points depend on."""
    h, w = dset.shape[-2:]
    lead = dset.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    r, c = np.asarray(rows_idx), np.asarray(cols_idx)
    if r.ndim != 1 or r.shape != c.shape or len(r) < 1 or r.dtype.kind not in "iu" or c.dtype.kind not in "iu":
        raise ValueError("rows_idx and cols_idx must be integer sequences of one length")
    r, c = r.astype(np.int64), c.astype(np.int64)
    r, c = np.where(r < 0, r + h, r), np.where(c < 0, c + w, c)          # (negative indices as numpy counts them)
    if r.min() < 0 or r.max() >= h or c.min() < 0 or c.max() >= w:
        raise IndexError(f"a point is outside the {h} x {w} frame")
    k = len(r)
    boxes = np.empty((n, k, 3), np.int64)
    boxes[:, :, 0] = np.arange(n)[:, None]
    boxes[:, :, 1] = r[None, :]
    boxes[:, :, 2] = c[None, :]
    got = read_boxes(dset, boxes.reshape(-1, 3), 1, 1, batch=batch, codec=codec)
    return got.reshape(tuple(lead) + (k,))
