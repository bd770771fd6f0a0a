"""CPU tests of ebcc_hip_time_ranks_check and ebcc_hip_time_ranks_work_bytes (include/ebcc_hip.h): everything the quantile decode
refuses before it touches a device, each refusal with a message, and the neighbour one step inside every limit accepted; and
the rank rule BatchCodec.quantiles applies on the host, against numpy.  The library loads without a device (as
test_window_plan.py relies on); a missing symbol is an AttributeError - a failure, not a skip."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import _lib as L

NO_BIN = 0xFFFFFFFF
NO_RANK = 2 ** 64 - 1
H, W = 64, 96


class TimeRanks(ctypes.Structure):
    """ebcc_hip_time_ranks"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t), ("n_ranks", ctypes.c_size_t),
                ("rank", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("count", ctypes.c_void_p)]


def check_fn():
    fn = L.product().ebcc_hip_time_ranks_check
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(TimeRanks), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]
    return fn


def bytes_fn():
    fn = L.product().ebcc_hip_time_ranks_work_bytes
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.POINTER(TimeRanks)]
    return fn


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


COUNT = np.zeros(8, np.uint64)
BINS = (0, 1, 1, 0, 2)                                 # bin 0: two frames, bin 1: two, bin 2: one, bin 3: none
RANKS = ((0, 1), (1, NO_RANK), (0, 0), (NO_RANK, NO_RANK))


class Spec:
    """a spec and the rank table it points to (the check never follows d_out: any address of the right alignment stands for it)"""

    def __init__(self, ranks=RANKS, rows=H, cols=W, n_bins=None, n_ranks=None, **fields):
        self.table = np.asarray(ranks, np.uint64)
        self.table = self.table.reshape(len(ranks), -1) if self.table.size else self.table.reshape(len(ranks), 0)
        nb = self.table.shape[0] if n_bins is None else n_bins
        nr = self.table.shape[1] if n_ranks is None else n_ranks
        self.c = TimeRanks(nb, rows, cols, nr, self.table.ctypes.data, 0x1000, COUNT.ctypes.data)
        for name, value in fields.items():
            setattr(self.c, name, value)


def run(s, bins=BINS, height=H, width=W, row0=0, col0=0, n_frames=None):
    b = None if bins is None else np.asarray(bins, np.uint32)
    n = len(b) if n_frames is None else n_frames
    return check_fn()(height, width, None if s is None else ctypes.byref(s.c), None if b is None else b.ctypes.data, n, row0, col0)


def refused(*args, word=None, **kw):
    got = run(*args, **kw)
    msg = last_error()
    return got == -1 and "ebcc_hip_time_ranks_check" in msg and (word is None or word in msg)


def test_accepts_and_counts_the_named_frames():
    assert run(Spec()) == 5
    assert run(Spec(), bins=[0, NO_BIN, 2, NO_BIN, NO_BIN, 1, 0, 1]) == 5
    assert run(Spec([[0, 6]]), bins=None, n_frames=7) == 7                    # (no bin list: every frame in bin 0; a rank of m - 1)
    assert run(Spec([[0]]), bins=[0]) == 1


def test_null_pointers():
    assert refused(None)
    for name in ("rank", "d_out", "count"):
        assert refused(Spec(**{name: None})), name


def test_zero_dimensions():
    for name in ("n_bins", "rows", "cols"):
        assert refused(Spec(**{name: 0}), word="zero"), name
    assert run(Spec(rows=1, cols=1)) == 5


def test_number_of_rank_slots():
    assert refused(Spec(n_ranks=0), word="n_ranks")
    assert refused(Spec([[0] * 17], n_ranks=17), bins=[0], word="n_ranks")
    assert run(Spec([[0] * 16]), bins=[0]) == 1


def test_ranks_against_the_frames_of_their_bin():
    assert run(Spec([[1, 0], [1, 1], [0, NO_RANK], [NO_RANK, NO_RANK]])) == 5             # (ranks of exactly m - 1)
    assert refused(Spec([[2, 0], [1, 1], [0, NO_RANK], [NO_RANK, NO_RANK]]), word="rank")   # bin 0 has two frames
    assert refused(Spec([[1, 0], [1, 1], [1, NO_RANK], [NO_RANK, NO_RANK]]), word="rank")   # bin 2 has one
    assert refused(Spec([[1, 0], [1, 1], [0, NO_RANK], [NO_RANK, 0]]), word="rank")         # bin 3 has none: only unused slots are legal
    assert refused(Spec([[NO_RANK, NO_RANK]] * 4), word="unused")                           # every slot unused
    assert run(Spec([[NO_RANK, NO_RANK]] * 3 + [[NO_RANK, 0]]), bins=[3]) == 1              # (bins 0 .. 2 empty and unused)
    assert refused(Spec([[NO_RANK - 1]]), bins=[0], word="rank")


def test_bins():
    assert refused(Spec(), bins=[0, 1, 4], word="bin")
    assert refused(Spec(), bins=[0, 1, NO_BIN - 1], word="bin")
    assert refused(Spec(), bins=[NO_BIN, NO_BIN], word="no frame")
    assert refused(Spec(), bins=[], n_frames=0, word="no frame")
    assert run(Spec([[0, NO_RANK]] + [[NO_RANK, NO_RANK]] * 3), bins=[NO_BIN, 0]) == 1


def test_a_bin_of_two_to_the_32_frames():
    one = Spec([[0]])
    assert run(one, bins=None, n_frames=2 ** 32 - 1) == 2 ** 32 - 1
    assert run(Spec([[2 ** 32 - 2]]), bins=None, n_frames=2 ** 32 - 1) == 2 ** 32 - 1
    assert refused(one, bins=None, n_frames=2 ** 32, word="2^32")


def test_window_inside_the_frame():
    assert run(Spec(rows=H, cols=W)) == 5                                    # (the window that is the frame)
    assert run(Spec(rows=40, cols=30), row0=H - 40, col0=W - 30) == 5        # (ends with the frame)
    assert refused(Spec(rows=40, cols=30), row0=H - 39, col0=0, word="window")
    assert refused(Spec(rows=40, cols=30), row0=0, col0=W - 29, word="window")
    assert refused(Spec(rows=H + 1, cols=W), word="window")
    assert refused(Spec(rows=H, cols=W + 1), word="window")
    assert refused(Spec(rows=1, cols=1), row0=H, col0=0, word="window")
    assert run(Spec(rows=1, cols=1), row0=H - 1, col0=W - 1) == 5
    assert refused(Spec(rows=1, cols=1), row0=2 ** 64 - 1, col0=0, word="window")         # (row0 + rows wraps)


def test_alignment_of_the_output():
    for off in (1, 2, 3):
        assert refused(Spec(d_out=0x3000 + off), word="aligned"), off
    assert run(Spec(d_out=0x3004)) == 5


@pytest.mark.parametrize("h,w,ok", [(2047, 2047, True), (2048, 96, False), (64, 2048, False), (0, 96, False), (64, 0, False)])
def test_geometry_of_the_frame(h, w, ok):
    s = Spec(rows=1, cols=1)
    if ok:
        assert run(s, height=h, width=w) == 5
    else:
        assert refused(s, height=h, width=w, word="geometry")


def test_sizes_that_overflow():
    assert refused(Spec(rows=2 ** 40, cols=2 ** 40), word="overflow")
    assert refused(Spec(rows=2 ** 31, cols=2 ** 31), word="overflow")        # (rows * cols fits, the workspace does not)
    assert refused(Spec(n_bins=2 ** 31, n_ranks=2), word="overflow")         # (a plane's number would not fit 32 bits)


def test_work_bytes():
    fn = bytes_fn()
    for n_bins, n_ranks, rows, cols in ((1, 1, 1, 1), (4, 2, H, W), (12, 3, 721, 1440), (3, 16, 37, 53)):
        s = Spec([[0] * n_ranks] * n_bins, rows=rows, cols=cols)
        assert fn(ctypes.byref(s.c)) == (16 + 2) * 4 * n_bins * n_ranks * rows * cols
    assert fn(ctypes.byref(Spec([[0] * 3] * 12, rows=721, cols=1440).c)) == 2691118080     # (the 2.7 GB of twelve months x three ranks)
    assert fn(None) == 0
    assert fn(ctypes.byref(Spec(rows=2 ** 40, cols=2 ** 40).c)) == 0
    assert fn(ctypes.byref(Spec(rows=2 ** 31, cols=2 ** 31).c)) == 0
    assert fn(ctypes.byref(Spec(rows=2 ** 29, cols=2 ** 28).c)) == 0         # (72 * 8 * 2^57 wraps)
    for name in ("n_bins", "rows", "cols", "n_ranks"):
        assert fn(ctypes.byref(Spec(**{name: 0}).c)) == 0, name
    assert fn(ctypes.byref(Spec(n_ranks=17).c)) == 0


# ---- the rank rule of BatchCodec.quantiles ----------------------------------------------------------------------------------
def np_quantile(a, q, method):
    if "method" in inspect.signature(np.quantile).parameters:
        return np.quantile(a, q, method=method)
    return np.quantile(a, q, interpolation=method)


@pytest.mark.parametrize("method", ["linear", "lower", "higher", "nearest"])
@pytest.mark.parametrize("m", [1, 2, 12])
def test_rank_rule_against_numpy(m, method):
    from ebcc_amd import h5_batch
    a = np.arange(m, dtype=np.float64)                                       # (the value at rank r is r)
    for q in (0, 0.25, 0.5, 0.75, 1):
        lo, hi, t = h5_batch.quantile_rule(q, m, method)
        assert 0 <= lo <= hi <= m - 1 and (method == "linear" or (lo == hi and t == 0))
        got = np.float64(a[lo] + (a[hi] - a[lo]) * t)
        assert got.tobytes() == np.float64(np_quantile(a, q, method)).tobytes(), (m, q, method, lo, hi, t)


def test_rank_rule_refusals():
    from ebcc_amd import h5_batch
    for q in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            h5_batch.quantile_rule(q, 5, "linear")
    with pytest.raises(ValueError):
        h5_batch.quantile_rule(0.5, 5, "midpoint")
    with pytest.raises(ValueError):
        h5_batch.quantile_rule(0.5, 0, "linear")
