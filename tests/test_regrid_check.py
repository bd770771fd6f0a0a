"""CPU tests of ebcc_hip_regrid_check (include/ebcc_hip.h): everything the regrid decode refuses before it touches a device,
each refusal with a message and the bounding box left untouched, the neighbour one step inside every limit accepted, and the
output size and the bounding box that come back.  The library loads without a device (as test_series_check.py relies on); a
missing symbol is an AttributeError - a failure, not a skip.

Not tested: an output size that overflows - n_out ends at 65535 per axis, so the product is below 2^32 floats on a 64-bit
size_t and the refusal cannot be reached through the interface."""
import ctypes

import numpy as np
import pytest

from ebcc_amd import regrid as M
from tests import _lib as L
from tests import _regrid as R

H, W = 64, 96


def check_fn():
    fn = L.product().ebcc_hip_regrid_check
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(R.RegridSpec), ctypes.POINTER(R.Region)]
    return fn


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


def raw_axis(first, count, weight=None, wrap=0, n_out=None, null=None):
    """an ebcc_hip_axis_map from plain lists, unchecked by Python -> (struct, what it points to)"""
    f, c = np.asarray(first, np.uint32), np.asarray(count, np.uint32)
    w = np.ones(int(c.astype(np.int64).sum()), np.float64) if weight is None else np.asarray(weight, np.float64)
    s = R.AxisMapC(len(f) if n_out is None else n_out, f.ctypes.data, c.ctypes.data, w.ctypes.data, wrap)
    if null:
        setattr(s, null, None)
    return s, (f, c, w)


def ident(n):
    return raw_axis(np.arange(n), np.ones(n))


def run(rows=None, cols=None, height=H, width=W, null_spec=False, want_box=True):
    """-> (return value, the box as a tuple); rows / cols: (struct, keep) of raw_axis, None: the identity"""
    rows, cols = rows or ident(height), cols or ident(width)
    spec = R.RegridSpec(rows[0], cols[0])
    box = R.Region(7, 7, 7, 7)
    got = check_fn()(height, width, None if null_spec else ctypes.byref(spec), ctypes.byref(box) if want_box else None)
    return got, (box.row0, box.col0, box.rows, box.cols)


def refused(**kw):
    got, box = run(**kw)
    return got == -1 and len(last_error()) > 0 and box == (7, 7, 7, 7)          # (and the box is not written)


def as_raw(m):
    return m.c_struct(), m


def test_sizes_and_bounding_boxes():
    assert run() == (H * W, (0, 0, H, W))                                        # the identity
    assert run(want_box=False)[0] == H * W                                        # (the box may be left out)
    # rows 10..50 x columns 20..70: a conservative map onto 8 x 5 cells
    rows = M.conservative_map(np.arange(H + 1.0), np.linspace(10.0, 50.0, 9))
    cols = M.conservative_map(np.arange(W + 1.0), np.linspace(20.0, 70.0, 6))
    assert run(as_raw(rows), as_raw(cols)) == (40, (10, 20, 40, 50))
    assert R.bounding(rows, cols, H, W) == (10, 20, 40, 50)
    # a flip reads what the forward map reads
    assert run(as_raw(M.flip_map(H)), as_raw(M.flip_map(W))) == (H * W, (0, 0, H, W))
    assert run(raw_axis([50, 30, 10], [1, 2, 3]), raw_axis([70, 20], [1, 1])) == (6, (10, 20, 41, 51))
    # a wrapping column map: the whole width, bounded rows
    cols = raw_axis([W - 2, 10], [5, 3], wrap=1)
    assert run(raw_axis([12, 20], [2, 4]), cols) == (4, (12, 0, 12, W))
    # wrap set, but no support crosses the seam: the box stays tight
    assert run(raw_axis([12], [2]), raw_axis([W - 5, 10], [5, 3], wrap=1)) == (2, (12, 10, 2, W - 10))
    # single positions
    assert run(raw_axis([H - 1], [1]), raw_axis([W - 1], [1])) == (1, (H - 1, W - 1, 1, 1))


def test_null_spec_and_null_tables():
    assert refused(null_spec=True)
    for name in ("first", "count", "weight"):
        assert refused(rows=raw_axis([0], [1], null=name)), name
        assert refused(cols=raw_axis([0], [1], null=name)), name


def test_number_of_outputs():
    assert refused(rows=raw_axis([0], [1], n_out=0))
    assert refused(cols=raw_axis([0], [1], n_out=0))
    n = 65535
    big = raw_axis(np.zeros(n), np.ones(n))
    assert run(rows=big, cols=raw_axis([0], [1]))[0] == n                          # one step inside the limit
    assert run(rows=raw_axis([0], [1]), cols=big)[0] == n
    over = raw_axis(np.zeros(n + 1), np.ones(n + 1))
    assert refused(rows=over) and refused(cols=over)


def test_tap_counts():
    h = w = 300
    assert refused(rows=raw_axis([0], [0]), height=h, width=w)
    assert refused(cols=raw_axis([0, 5], [1, 0]), height=h, width=w)
    assert "output 1" in last_error()
    assert run(rows=raw_axis([0], [256]), cols=raw_axis([44], [256]), height=h, width=w) == (1, (0, 44, 256, 256))     # the limit itself
    assert refused(rows=raw_axis([0], [257]), height=h, width=w)
    assert refused(cols=raw_axis([0], [257]), height=h, width=w)
    assert refused(cols=raw_axis([0], [257], wrap=1), height=h, width=w)           # (wrapping does not lift the limit)


def test_supports_inside_the_axis():
    assert run(rows=raw_axis([H - 3], [3]))[0] == W                               # ends on the last index
    assert run(cols=raw_axis([W - 3], [3]))[0] == H
    assert refused(rows=raw_axis([H - 3], [4]))
    assert refused(cols=raw_axis([W - 3], [4]))
    assert run(cols=raw_axis([W - 3], [4], wrap=1)) == (H, (0, 0, H, W))          # with wrap it is a map
    assert refused(rows=raw_axis([H], [1]))                                        # first >= extent
    assert refused(cols=raw_axis([W], [1]))
    assert refused(cols=raw_axis([W], [1], wrap=1))                                # (also with wrap)
    assert refused(cols=raw_axis([2 ** 32 - 1], [2], wrap=1))
    assert refused(rows=raw_axis([2 ** 32 - 1], [2]))                              # (first + count wraps in 32 bits)
    assert refused(rows=raw_axis([0, H - 1], [1, 2]))
    assert "output 1" in last_error()
    assert run(cols=raw_axis([5], [200], wrap=1), width=9, height=4) == (4, (0, 0, 4, 9))    # round the axis many times


def test_wrap_on_the_row_map():
    assert refused(rows=raw_axis([0], [1], wrap=1))
    assert refused(rows=raw_axis([H - 1], [2], wrap=1))


def test_weights():
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 2, 5):
            w = np.ones(6)
            w[at] = bad
            assert refused(rows=raw_axis([0, 9], [2, 4], w)), (bad, at)
            assert refused(cols=raw_axis([0, 9], [2, 4], w)), (bad, at)
    for good in (0.0, -0.0, -1.0, 5e-324, -1e300):
        w = np.ones(6)
        w[5] = good
        assert run(rows=raw_axis([0, 9], [2, 4], w))[0] == 2 * W, good


@pytest.mark.parametrize("h,w,ok", [(2047, 2047, True), (2048, 96, False), (64, 2048, False), (0, 96, False), (64, 0, False), (1, 1, True)])
def test_geometry_of_the_frame(h, w, ok):
    one = dict(rows=raw_axis([0], [1]), cols=raw_axis([0], [1]))
    if ok:
        assert run(height=h, width=w, **one) == (1, (0, 0, 1, 1))
    else:
        assert refused(height=h, width=w, **one)


def test_messages_name_the_call():
    assert run(rows=raw_axis([H - 3], [4]))[0] == -1
    assert "ebcc_hip_regrid_check" in last_error() and "row output 0" in last_error()
