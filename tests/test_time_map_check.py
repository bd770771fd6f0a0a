"""CPU tests of ebcc_hip_time_map_check (include/ebcc_hip.h): everything the time-map decode refuses before it touches a device,
each refusal with a message that names the function, and the neighbour one step inside every limit accepted; h5_batch's
time_map_terms against that check on the same inputs; and trend_weights / running_mean_weights against their formulae.  The
library loads without a device (as test_quantile_check.py relies on); a missing symbol is an AttributeError - a failure, not a
skip."""
import ctypes

import numpy as np
import pytest

from tests import _lib as L

H, W = 64, 96


class TimeMap(ctypes.Structure):
    """ebcc_hip_time_map"""
    _fields_ = [("n_out", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t), ("start", ctypes.c_void_p),
                ("frame", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("d_acc", ctypes.c_void_p), ("count", ctypes.c_void_p)]


def check_fn():
    fn = L.product().ebcc_hip_time_map_check
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(TimeMap), ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]
    return fn


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


COUNT = np.zeros(8, np.uint64)
# three outputs over five frames: a dense one, a sparse one that shares frames with it, one without terms; frame 2 is unnamed
START = (0, 4, 6, 6)
FRAME = (0, 1, 3, 4, 1, 4)
WEIGHT = (0.5, -2.0 / 7.0, 0.1, 1.0 / 3.0, 0.0, -1e300)           # (a weight of 0 is a term like any other)
N_FRAMES = 5


class Spec:
    """a map and the arrays it points to (the check never follows d_acc: any address of the right alignment stands for it)"""

    def __init__(self, start=START, frame=FRAME, weight=WEIGHT, rows=H, cols=W, n_out=None, **fields):
        self.start, self.frame, self.weight = np.asarray(start, np.uint64), np.asarray(frame, np.uint32), np.asarray(weight, np.float64)
        self.c = TimeMap(len(self.start) - 1 if n_out is None else n_out, rows, cols, self.start.ctypes.data, self.frame.ctypes.data,
                         self.weight.ctypes.data, 0x1000, COUNT.ctypes.data)
        for name, value in fields.items():
            setattr(self.c, name, value)


def run(s, n_frames=N_FRAMES, height=H, width=W, row0=0, col0=0):
    return check_fn()(height, width, None if s is None else ctypes.byref(s.c), n_frames, row0, col0)


def refused(*args, word=None, **kw):
    got = run(*args, **kw)
    msg = last_error()
    return got == -1 and "ebcc_hip_time_map_check" in msg and (word is None or word in msg)


def test_accepts_and_counts_the_distinct_frames():
    assert run(Spec()) == 4                                        # frames 0, 1, 3, 4: 1 and 4 are named twice, 2 by nobody
    assert run(Spec(), n_frames=1000) == 4
    assert run(Spec((0, 1), (0,), (1.0,)), n_frames=1) == 1
    assert run(Spec((0, 3, 6, 9), (0, 1, 2) * 3, (1.0,) * 9), n_frames=3) == 3          # three outputs that name the same frames
    # (a frame axis much longer than the list: the distinct frames are counted by sorting)
    assert run(Spec((0, 2, 4), (5, 2 ** 32 - 2, 5, 7), (1.0,) * 4), n_frames=2 ** 32 - 1) == 3


def test_null_pointers():
    assert refused(None)
    for name in ("start", "d_acc", "count", "frame", "weight"):
        s = Spec()
        setattr(s.c, name, None)
        assert refused(s), name


def test_zero_dimensions():
    for name in ("n_out", "rows", "cols"):
        assert refused(Spec(**{name: 0}), word="zero"), name
    assert run(Spec(rows=1, cols=1)) == 4


def test_start():
    assert refused(Spec((1, 4, 6, 6)), word="start[0]")
    assert refused(Spec((0, 4, 3, 6)), word="decreases")
    assert run(Spec((0, 4, 4, 6))) == 4                            # (equal neighbours: an output without terms)
    assert refused(Spec((0, 0, 0, 0)), word="no term")
    assert run(Spec((0, 0, 0, 1), (2,), (1.0,))) == 1              # (one term, in the last output)


def test_frames():
    assert refused(Spec(), n_frames=4, word="frame")                                     # frame 4 of 4
    assert run(Spec(), n_frames=5) == 4
    assert refused(Spec(frame=(0, 1, 1, 4, 1, 4)), word="increasing")                   # a frame twice in an output
    assert refused(Spec(frame=(0, 3, 1, 4, 1, 4)), word="increasing")                   # out of order
    assert refused(Spec(frame=(0, 1, 3, 4, 4, 1)), word="increasing")                   # in the second output
    assert run(Spec(frame=(0, 1, 3, 4, 0, 4))) == 4                                     # (output 1 may begin below output 0's last)
    assert refused(Spec(), n_frames=0, word="frame")


def test_weights_must_be_finite():
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 5):
            w = list(WEIGHT)
            w[at] = bad
            assert refused(Spec(weight=w), word="finite"), (bad, at)
    w = list(WEIGHT)
    w[0] = np.finfo(np.float64).max
    assert run(Spec(weight=w)) == 4


def test_alignment_of_the_accumulators():
    for off in range(1, 8):
        assert refused(Spec(d_acc=0x3000 + off), word="aligned"), off
    assert run(Spec(d_acc=0x3008)) == 4


def test_window_inside_the_frame():
    assert run(Spec(rows=H, cols=W)) == 4                                    # (the window that is the frame)
    assert run(Spec(rows=40, cols=30), row0=H - 40, col0=W - 30) == 4        # (ends with the frame)
    assert refused(Spec(rows=40, cols=30), row0=H - 39, col0=0, word="window")
    assert refused(Spec(rows=40, cols=30), row0=0, col0=W - 29, word="window")
    assert refused(Spec(rows=H + 1, cols=W), word="window")
    assert refused(Spec(rows=H, cols=W + 1), word="window")
    assert refused(Spec(rows=1, cols=1), row0=H, col0=0, word="window")
    assert run(Spec(rows=1, cols=1), row0=H - 1, col0=W - 1) == 4
    assert refused(Spec(rows=1, cols=1), row0=2 ** 64 - 1, col0=0, word="window")         # (row0 + rows wraps)


@pytest.mark.parametrize("h,w,ok", [(2047, 2047, True), (2048, 96, False), (64, 2048, False), (0, 96, False), (64, 0, False)])
def test_geometry_of_the_frame(h, w, ok):
    s = Spec(rows=1, cols=1)
    if ok:
        assert run(s, height=h, width=w) == 4
    else:
        assert refused(s, height=h, width=w, word="geometry")


def test_sizes_that_overflow():
    assert refused(Spec(rows=2 ** 40, cols=2 ** 40), word="overflow")
    assert refused(Spec(rows=2 ** 31, cols=2 ** 30), word="overflow")        # (rows * cols fits, times 8 bytes does not)
    assert refused(Spec(n_out=2 ** 32 - 1), word="overflow")                 # (an output's number would not fit 32 bits)
    assert refused(Spec(), n_frames=2 ** 63, word="too many")
    assert run(Spec(), n_frames=2 ** 63 - 1) == 4


# ---- time_map_terms against the C check -----------------------------------------------------------------------------------------
TRIPLES = [
    (START, FRAME, WEIGHT, True),
    ((1, 4, 6, 6), FRAME, WEIGHT, False),
    ((0, 4, 3, 6), FRAME, WEIGHT, False),
    ((0, 0, 0, 0), FRAME, WEIGHT, False),
    ((0, 4, 4, 6), FRAME, WEIGHT, True),
    (START, (0, 1, 1, 4, 1, 4), WEIGHT, False),
    (START, (0, 1, 3, 4, 4, 1), WEIGHT, False),
    (START, (0, 1, 3, 4, 0, 4), WEIGHT, True),
    (START, (0, 1, 3, 5, 1, 4), WEIGHT, False),                   # frame 5 of 5
    (START, FRAME, (0.5, np.nan, 0.1, 1.0, 0.0, 1.0), False),
    (START, FRAME, (0.5, 1.0, 0.1, 1.0, 0.0, -np.inf), False),
    ((0, 1), (4,), (2.5,), True),
]


@pytest.mark.parametrize("k", range(len(TRIPLES)))
def test_terms_match_the_c_check(k):
    from ebcc_amd import h5_batch
    start, frame, weight, ok = TRIPLES[k]
    c = run(Spec(start, frame, weight))
    assert (c >= 0) == ok, last_error()
    if ok:
        s, f, w = h5_batch.time_map_terms((start, frame, weight), n_frames=N_FRAMES)
        assert (s.dtype, f.dtype, w.dtype) == (np.uint64, np.uint32, np.float64)
        assert s.tolist() == list(start) and f.tolist() == list(frame) and w.tobytes() == np.asarray(weight, np.float64).tobytes()
        assert c == len(set(frame[:start[-1]]))
    else:
        with pytest.raises(ValueError):
            h5_batch.time_map_terms((start, frame, weight), n_frames=N_FRAMES)


def test_terms_of_a_dense_array():
    from ebcc_amd import h5_batch
    dense = np.array([[0.5, -2, 0, 0.25, 1], [0, 3, 0, 0, -1], [0, 0, 0, 0, 0]], np.float32)
    s, f, w = h5_batch.time_map_terms(dense)
    assert s.tolist() == [0, 4, 6, 6] and f.tolist() == [0, 1, 3, 4, 1, 4] and w.tolist() == [0.5, -2, 0.25, 1, 3, -1]
    assert run(Spec(s, f, w)) == 4
    assert h5_batch.time_map_terms(dense.astype(np.int32))[2].dtype == np.float64
    for bad in (np.zeros((2, 5)), np.array([[1.0, np.nan]]), np.array([[np.inf, 1.0]]), np.zeros(5), np.zeros((0, 5))):
        with pytest.raises(ValueError):
            h5_batch.time_map_terms(bad)
    with pytest.raises(ValueError):
        h5_batch.time_map_terms(dense, n_frames=6)


# ---- the two example maps -------------------------------------------------------------------------------------------------------
def test_trend_weights_match_the_formula_and_polyfit():
    from ebcc_amd import h5_batch
    r = np.random.default_rng(7)
    for t in (np.arange(12.0), np.array([1979.5, 1980.25, 1983.0, 1990.75, 2001.0, 2001.5, 2020.0])):
        n = len(t)
        w = h5_batch.trend_weights(t)
        assert w.shape == (2, n) and w.dtype == np.float64
        c = t - t.mean()
        assert w[0].tobytes() == np.full(n, 1.0 / n).tobytes()
        assert w[1].tobytes() == (c / (c * c).sum()).tobytes()
        series = r.standard_normal(n) * 3 + 0.7 * (t - t[0]) + 280.0
        got = w @ series
        slope = np.polyfit(t - t.mean(), series, 1)[0]
        # float64 round-off, not the device: a sum of n terms w_i * s_i in any order is within n * eps * sum |w_i * s_i| of the
        # exact one, and sum |w_i * s_i| <= n * max |w| * max |s|; 8 of those for the two sides and polyfit's own solve
        eps, big = np.finfo(np.float64).eps, np.abs(series).max()
        assert np.isclose(got[0], series.mean(), rtol=0, atol=8 * n * eps * big)
        assert np.isclose(got[1], slope, rtol=0, atol=8 * n * eps * n * np.abs(w[1]).max() * big)
    for bad in ([1.0], [2.0, 2.0], [1.0, np.nan], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            h5_batch.trend_weights(bad)


def test_running_mean_weights_match_the_formula():
    from ebcc_amd import h5_batch
    for n, width in ((9, 3), (5, 5), (4, 1)):
        w = h5_batch.running_mean_weights(n, width)
        assert w.shape == (n - width + 1, n) and w.dtype == np.float64
        for o in range(n - width + 1):
            want = np.zeros(n)
            want[o:o + width] = 1.0 / width
            assert w[o].tobytes() == want.tobytes()
        s, f, _ = h5_batch.time_map_terms(w)
        assert s.tolist() == [o * width for o in range(n - width + 2)] and f.tolist() == [o + j for o in range(n - width + 1) for j in range(width)]
    for n, width in ((4, 5), (4, 0)):
        with pytest.raises(ValueError):
            h5_batch.running_mean_weights(n, width)
