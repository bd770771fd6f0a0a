"""CPU tests of ebcc_hip_pair_stats_check (include/ebcc_hip.h): everything the pair decode refuses before it touches a device,
each refusal with a message that names the call, and the neighbour one step inside every limit accepted.  The library loads
without a device (as test_window_plan.py relies on); a missing symbol is an AttributeError - a failure, not a skip."""
import ctypes

import numpy as np
import pytest

from tests import _lib as L

NO_BIN = 0xFFFFFFFF
H, W = 64, 96
CALL = "ebcc_hip_pair_stats_check"


class PairStats(ctypes.Structure):
    """ebcc_hip_pair_stats"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("d_sum_x", ctypes.c_void_p), ("d_sum_y", ctypes.c_void_p), ("d_sum_xx", ctypes.c_void_p), ("d_sum_yy", ctypes.c_void_p),
                ("d_sum_xy", ctypes.c_void_p), ("d_sum_mag", ctypes.c_void_p), ("d_max_mag", ctypes.c_void_p), ("d_over_mag", ctypes.c_void_p),
                ("threshold", ctypes.c_float), ("count", ctypes.c_void_p)]


def check_fn():
    fn = L.product().ebcc_hip_pair_stats_check
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(PairStats), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]
    return fn


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


COUNT = np.zeros(8, np.uint64)
# (the check never follows a device pointer: any address of the right alignment stands for one)
DOUBLES = ("d_sum_x", "d_sum_y", "d_sum_xx", "d_sum_yy", "d_sum_xy", "d_sum_mag")
WORDS = ("d_max_mag", "d_over_mag")
FIELDS = DOUBLES + WORDS


def stats(n_bins=4, rows=H, cols=W, count=True, threshold=0.5, **ptrs):
    s = PairStats(n_bins, rows, cols, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, threshold, COUNT.ctypes.data if count else None)
    for name, value in ptrs.items():
        setattr(s, name, value)
    return s


def run(s, bins=(0, 1, 1, 0, 2), height=H, width=W, row0=0, col0=0, n_steps=None):
    b = None if bins is None else np.asarray(bins, np.uint32)
    n = len(b) if n_steps is None else n_steps
    return check_fn()(height, width, None if s is None else ctypes.byref(s), None if b is None else b.ctypes.data, n, row0, col0)


def refused(*args, **kw):
    """-1, with a message that names the call"""
    got = run(*args, **kw)
    return got == -1 and CALL in last_error() and len(last_error()) > len(CALL) + 2


def test_struct_layout():
    assert ctypes.sizeof(PairStats) == 13 * 8 and PairStats.threshold.offset == 11 * 8 and PairStats.count.offset == 12 * 8


def test_accepts_and_counts_the_named_steps():
    assert run(stats()) == 5
    assert run(stats(), bins=[0, NO_BIN, 3, NO_BIN, NO_BIN, 1]) == 3
    assert run(stats(), bins=None, n_steps=7) == 7                           # (no bin list: every step in bin 0)
    assert run(stats(n_bins=1), bins=[0]) == 1


def test_null_stats_and_null_count():
    assert refused(None)
    assert refused(stats(count=False))


def test_every_device_array_null():
    assert refused(stats(**{name: None for name in FIELDS}))
    for keep in FIELDS:                                                      # (one is enough)
        assert run(stats(**{name: None for name in FIELDS if name != keep})) == 5, keep


def test_zero_dimensions():
    for name in ("n_bins", "rows", "cols"):
        assert refused(stats(**{name: 0})), name
    assert run(stats(n_bins=3, rows=1, cols=1)) == 5


def test_window_inside_the_frame():
    assert run(stats(rows=40, cols=30), row0=H - 40, col0=W - 30) == 5      # (ends with the frame)
    assert refused(stats(rows=40, cols=30), row0=H - 39, col0=0)
    assert refused(stats(rows=40, cols=30), row0=0, col0=W - 29)
    assert refused(stats(rows=H + 1, cols=W))
    assert refused(stats(rows=H, cols=W + 1))
    assert refused(stats(rows=1, cols=1), row0=H, col0=0)
    assert refused(stats(rows=1, cols=1), row0=0, col0=W)
    assert run(stats(rows=1, cols=1), row0=H - 1, col0=W - 1) == 5
    assert refused(stats(rows=1, cols=1), row0=2 ** 64 - 1, col0=0)         # (row0 + rows wraps)
    assert refused(stats(rows=1, cols=1), row0=0, col0=2 ** 64 - 1)


def test_alignment():
    for name in DOUBLES:
        assert refused(stats(**{name: 0x1004})), name                        # (4-byte aligned is not enough for doubles)
        assert run(stats(**{name: 0x1008})) == 5, name
    for name in WORDS:
        for off in (1, 2, 3):
            assert refused(stats(**{name: 0x3000 + off})), (name, off)
        assert run(stats(**{name: 0x3004})) == 5, name


def test_threshold():
    assert refused(stats(threshold=float("nan")))
    assert run(stats(threshold=float("nan"), d_over_mag=None)) == 5         # (not looked at without d_over_mag)
    assert run(stats(threshold=float("inf"))) == 5
    assert run(stats(threshold=-1.0)) == 5


def test_bins():
    assert refused(stats(n_bins=4), bins=[0, 1, 4])
    assert run(stats(n_bins=4), bins=[0, 1, 3]) == 3
    assert refused(stats(n_bins=4), bins=[0, 1, NO_BIN - 1])
    assert refused(stats(), bins=[NO_BIN, NO_BIN])                           # (no step named)
    assert refused(stats(), bins=[], n_steps=0)
    assert run(stats(), bins=[NO_BIN, 2]) == 1


@pytest.mark.parametrize("h,w,ok", [(2047, 2047, True), (2048, 96, False), (64, 2048, False), (0, 96, False), (64, 0, False)])
def test_geometry_of_the_frame(h, w, ok):
    s = stats(rows=1, cols=1)
    if ok:
        assert run(s, height=h, width=w) == 5
    else:
        assert refused(s, height=h, width=w)


def test_messages_say_what_is_wrong():
    assert run(stats(n_bins=2), bins=[0, 2]) == -1
    assert CALL in last_error() and "bin" in last_error() and "step 1" in last_error()
    assert run(stats(d_sum_xy=0x1004)) == -1
    assert "d_sum_xy" in last_error() and "8-byte" in last_error()
    assert run(stats(threshold=float("nan"))) == -1
    assert "threshold" in last_error()
