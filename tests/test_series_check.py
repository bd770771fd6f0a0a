"""CPU tests of ebcc_hip_area_check (include/ebcc_hip.h): everything the area series refuses before it touches a device, each
refusal with a message, the neighbour one step inside every limit accepted, and the bounding box that comes back.  The library
loads without a device (as test_reduce_check.py relies on); a missing symbol is an AttributeError - a failure, not a skip.

Not tested: the neighbour inside the limit on n_regions - a list of 2^57 regions does not fit into memory."""
import ctypes

import numpy as np
import pytest

from tests import _lib as L
from tests import _series as S

H, W = 64, 96


def check_fn():
    fn = L.product().ebcc_hip_area_check
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(S.AreaSpec), ctypes.POINTER(S.Region)]
    return fn


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


ONE = [(0, 0, H, W)]
# (the check never follows the device pointer: any address of the right alignment stands for one)


def run(regions=ONE, w_row=None, d_w_pix=None, height=H, width=W, n_regions=None, null_list=False, null_spec=False, want_box=True):
    """-> (return value, bounding box as a tuple or None)"""
    arr = S.region_array(regions) if regions else None
    wr = None if w_row is None else np.ascontiguousarray(w_row, np.float64)
    spec = S.AreaSpec(len(regions) if n_regions is None else n_regions, None if null_list or arr is None else ctypes.addressof(arr),
                      None if wr is None else wr.ctypes.data, d_w_pix, 1, 0.5)
    box = S.Region(7, 7, 7, 7)
    got = check_fn()(height, width, None if null_spec else ctypes.byref(spec), ctypes.byref(box) if want_box else None)
    return got, (box.row0, box.col0, box.rows, box.cols)


def refused(**kw):
    got, box = run(**kw)
    return got == -1 and len(last_error()) > 0 and box == (7, 7, 7, 7)          # (and the box is not written)


def test_accepts_and_returns_the_bounding_box():
    assert run() == (1, (0, 0, H, W))
    assert run(regions=[(3, 5, 10, 20)]) == (1, (3, 5, 10, 20))
    assert run(regions=[(3, 50, 10, 20), (40, 5, 4, 6)]) == (2, (3, 5, 41, 65))
    assert run(regions=[(0, 0, 1, 1), (H - 1, W - 1, 1, 1)]) == (2, (0, 0, H, W))      # two corners: the frame
    assert run(regions=[(9, 9, 5, 5), (9, 9, 5, 5), (10, 10, 2, 2)]) == (3, (9, 9, 5, 5))   # a repeat, one inside another
    assert run(regions=[(3, 5, 10, 20)], want_box=False)[0] == 1                      # (the box may be left out)
    assert run(w_row=np.ones(H), d_w_pix=0x1000)[0] == 1


def test_null_spec_null_list_and_no_regions():
    assert refused(null_spec=True)
    assert refused(null_list=True)
    assert refused(regions=[], n_regions=0)
    assert refused(n_regions=0)                                                      # (a list, but none of it)


def test_regions_inside_the_frame():
    assert run(regions=[(H - 40, W - 30, 40, 30)])[0] == 1                            # (ends with the frame)
    assert refused(regions=[(H - 39, 0, 40, 30)])
    assert refused(regions=[(0, W - 29, 40, 30)])
    assert refused(regions=[(0, 0, H + 1, W)])
    assert refused(regions=[(0, 0, H, W + 1)])
    assert refused(regions=[(H, 0, 1, 1)])
    assert refused(regions=[(0, W, 1, 1)])
    assert run(regions=[(H - 1, W - 1, 1, 1)])[0] == 1
    assert refused(regions=[(2 ** 64 - 1, 0, 2, 1)])                                 # (row0 + rows wraps)
    assert refused(regions=[(0, 2 ** 64 - 1, 1, 2)])
    assert refused(regions=[(0, 0, 0, 5)])                                           # empty
    assert refused(regions=[(0, 0, 5, 0)])
    assert refused(regions=[ONE[0], (0, 0, 5, 0)])                                   # (the second of two)
    assert "region 1" in last_error()


def test_row_weights():
    for bad in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        for at in (0, H // 2, H - 1):
            w = np.ones(H)
            w[at] = bad
            assert refused(w_row=w), (bad, at)
    for good in (0.0, -0.0, 5e-324, 1e300):
        w = np.ones(H)
        w[H - 1] = good
        assert run(w_row=w)[0] == 1, good
    # every entry of the frame is looked at, not only the rows of the regions
    w = np.ones(H)
    w[H - 1] = np.nan
    assert refused(regions=[(0, 0, 4, 4)], w_row=w)


def test_alignment_of_the_pixel_weights():
    for off in (1, 2, 3):
        assert refused(d_w_pix=0x3000 + off), off
    assert run(d_w_pix=0x3004)[0] == 1


@pytest.mark.parametrize("h,w,ok", [(2047, 2047, True), (2048, 96, False), (64, 2048, False), (0, 96, False), (64, 0, False), (1, 1, True)])
def test_geometry_of_the_frame(h, w, ok):
    if ok:
        assert run(regions=[(0, 0, 1, 1)], height=h, width=w) == (1, (0, 0, 1, 1))
    else:
        assert refused(regions=[(0, 0, 1, 1)], height=h, width=w)


def test_sizes_that_overflow():
    # (refused before the list is followed: it holds one region)
    assert refused(n_regions=2 ** 63)                                                # more than a long counts
    assert refused(n_regions=2 ** 62)                                                # the table's bytes wrap
    assert refused(n_regions=2 ** 64 - 1)


def test_messages_name_the_call():
    assert run(regions=[(0, 0, H + 1, W)])[0] == -1
    assert "ebcc_hip_area_check" in last_error() and "region 0" in last_error()
