"""CPU tests of ebcc_hip_time_stats_check (include/ebcc_hip.h): everything the reduce decode refuses before it touches a device,
each refusal with a message, and the neighbour one step inside every limit accepted.  The library loads without a device (as
test_window_plan.py relies on); a missing symbol is an AttributeError - a failure, not a skip."""
import ctypes

import numpy as np
import pytest

from tests import _lib as L

NO_BIN = 0xFFFFFFFF
H, W = 64, 96


class TimeStats(ctypes.Structure):
    """ebcc_hip_time_stats"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("d_sum", ctypes.c_void_p), ("d_sum_sq", ctypes.c_void_p), ("d_min", ctypes.c_void_p), ("d_max", ctypes.c_void_p),
                ("d_over", ctypes.c_void_p), ("threshold", ctypes.c_float), ("count", ctypes.c_void_p)]


def check_fn():
    fn = L.product().ebcc_hip_time_stats_check
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(TimeStats), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]
    return fn


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


COUNT = np.zeros(8, np.uint64)
# (the check never follows a device pointer: any address of the right alignment stands for one)
FIELDS = ("d_sum", "d_sum_sq", "d_min", "d_max", "d_over")


def stats(n_bins=4, rows=H, cols=W, count=True, **ptrs):
    s = TimeStats(n_bins, rows, cols, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0.5, COUNT.ctypes.data if count else None)
    for name, value in ptrs.items():
        setattr(s, name, value)
    return s


def run(s, bins=(0, 1, 1, 0, 2), height=H, width=W, row0=0, col0=0, n_frames=None):
    b = None if bins is None else np.asarray(bins, np.uint32)
    n = len(b) if n_frames is None else n_frames
    return check_fn()(height, width, None if s is None else ctypes.byref(s), None if b is None else b.ctypes.data, n, row0, col0)


def refused(*args, **kw):
    got = run(*args, **kw)
    return got == -1 and len(last_error()) > 0


def test_accepts_and_counts_the_named_frames():
    assert run(stats()) == 5
    assert run(stats(), bins=[0, NO_BIN, 3, NO_BIN, NO_BIN, 1]) == 3
    assert run(stats(), bins=None, n_frames=7) == 7                          # (no bin list: every frame in bin 0)
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


def test_alignment():
    for name in ("d_sum", "d_sum_sq"):
        assert refused(stats(**{name: 0x1004})), name                        # (4-byte aligned is not enough for doubles)
        assert run(stats(**{name: 0x1008})) == 5, name
    for name in ("d_min", "d_max", "d_over"):
        for off in (1, 2, 3):
            assert refused(stats(**{name: 0x3000 + off})), (name, off)
        assert run(stats(**{name: 0x3004})) == 5, name


def test_bins():
    assert refused(stats(n_bins=4), bins=[0, 1, 4])
    assert run(stats(n_bins=4), bins=[0, 1, 3]) == 3
    assert refused(stats(n_bins=4), bins=[0, 1, NO_BIN - 1])
    assert refused(stats(), bins=[NO_BIN, NO_BIN])                           # (no frame named)
    assert refused(stats(), bins=[], n_frames=0)
    assert run(stats(), bins=[NO_BIN, 2]) == 1


@pytest.mark.parametrize("h,w,ok", [(2047, 2047, True), (2048, 96, False), (64, 2048, False), (0, 96, False), (64, 0, False)])
def test_geometry_of_the_frame(h, w, ok):
    s = stats(rows=1, cols=1)
    if ok:
        assert run(s, height=h, width=w) == 5
    else:
        assert refused(s, height=h, width=w)


def test_messages_name_the_call():
    assert run(stats(n_bins=2), bins=[0, 2]) == -1
    assert "ebcc_hip_time_stats_check" in last_error() and "bin" in last_error()
