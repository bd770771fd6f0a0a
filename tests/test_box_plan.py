"""CPU tests of the box-list decode's plan (ebcc_hip_boxes_plan, include/ebcc_hip.h): per frame, the code-blocks a decode of
a list of boxes reads - the OR of what ebcc_hip_window_plan keeps for the boxes of that frame (tests/test_window_plan.py holds
that plan between a float64 model and the radius-4 cone), nothing for a frame no box names.  The library loads without a
device; a missing symbol fails."""
import ctypes

import numpy as np
import pytest

from tests import _lib as L
from tests import test_window_plan as P

GEOMETRIES = [(64, 96), (100, 130), (97, 131), (721, 1440)]
N_FRAMES = 9


def _fn():
    fn = getattr(L.product(), "ebcc_hip_boxes_plan")      # AttributeError where the feature is missing: a failure, not a skip
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_size_t] * 3 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    return fn


def boxes_plan(h, w, n_frames, boxes, rows, cols, with_keep=True):
    """-> (return value, keep [n_frames][blocks] or None); a refused call must leave keep as it was"""
    table = np.ascontiguousarray(np.asarray(boxes, np.uint64).reshape(-1, 3))      # == ebcc_hip_box[]
    n = _fn()(h, w, n_frames, table.ctypes.data if len(table) else None, len(table), rows, cols, None, 0)
    if not with_keep or n < 0:
        if n < 0:
            blocks = len(P.block_list(h, w))
            keep = np.full((max(n_frames, 1), blocks), 0x5A, np.uint8)
            assert _fn()(h, w, n_frames, table.ctypes.data if len(table) else None, len(table), rows, cols, keep.ctypes.data, blocks) == -1
            assert (keep == 0x5A).all(), "keep written by a call that refuses"
        return n, None
    keep = np.full((n_frames, n), 0x5A, np.uint8)
    assert _fn()(h, w, n_frames, table.ctypes.data, len(table), rows, cols, keep.ctypes.data, n) == n
    return n, keep


def window_keep(h, w, win):
    n, _, blocks = P.plan(h, w, *win)
    assert n > 0
    return blocks[:, 5].astype(np.uint8)


def seeded_lists(h, w):
    """(rows, cols, boxes sorted by frame): a few sizes, boxes spread over some of the frames - repeats, overlaps, frames
    without a box"""
    rng = np.random.default_rng(7 * h + w)
    out = []
    for rows, cols in [(1, 1), (min(h, 19), min(w, 23)), (min(h, 64), min(w, 65)), (h, w), (1, w), (h, 1)]:
        named = sorted(rng.choice(N_FRAMES, size=int(rng.integers(1, N_FRAMES)), replace=False))
        boxes = []
        for f in named:
            for _ in range(int(rng.integers(1, 6))):
                boxes.append((int(f), int(rng.integers(0, h - rows + 1)), int(rng.integers(0, w - cols + 1))))
            if rng.random() < 0.5:
                boxes.append(boxes[-1])                               # an identical box
        boxes += [(named[-1], 0, 0), (named[-1], h - rows, w - cols)]  # corners
        out.append((rows, cols, boxes))
    return out


@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_keep_is_the_or_of_the_window_plans(h, w):
    for rows, cols, boxes in seeded_lists(h, w):
        n, keep = boxes_plan(h, w, N_FRAMES, boxes, rows, cols)
        assert n == len(P.block_list(h, w))
        want = np.zeros((N_FRAMES, n), np.uint8)
        for f, r0, c0 in boxes:
            want[f] |= window_keep(h, w, (r0, c0, rows, cols))
        assert np.array_equal(keep, want), (rows, cols)
        named = {f for f, _, _ in boxes}
        for f in range(N_FRAMES):
            assert (f in named) == bool(keep[f].any()), f                # an unnamed frame: all zeros; a named one keeps something
        assert boxes_plan(h, w, N_FRAMES, boxes, rows, cols, with_keep=False)[0] == n


def test_points_keep_few_code_blocks():
    # (a plan that keeps everything would pass above only if the window plan did: 64 points of a 721 x 1440 frame need a part)
    rng = np.random.default_rng(3)
    boxes = [(0, int(rng.integers(0, 721)), int(rng.integers(0, 1440))) for _ in range(4)]
    n, keep = boxes_plan(721, 1440, 2, boxes, 1, 1)
    assert n == 298 and 0 < int(keep[0].sum()) < 150 and not keep[1].any()


@pytest.mark.parametrize("h,w", [(100, 130), (721, 1440)])
def test_refusals(h, w):
    big = (1 << 64) - 1
    ok = [(0, 0, 0), (1, 5, 5), (1, 5, 5), (3, h - 10, w - 10)]
    assert boxes_plan(h, w, 4, ok, 10, 10)[0] > 0
    bad = [
        ("no boxes", 4, [], 10, 10),
        ("rows zero", 4, ok, 0, 10), ("cols zero", 4, ok, 10, 0),
        ("box below the frame", 4, ok[:3] + [(3, h - 9, 0)], 10, 10), ("box right of the frame", 4, ok[:3] + [(3, 0, w - 9)], 10, 10),
        ("box larger than the frame", 4, [(0, 0, 0)], h + 1, 1), ("box wider than the frame", 4, [(0, 0, 0)], 1, w + 1),
        ("origin that wraps", 4, [(0, big, 0)], 2, 1), ("origin that wraps", 4, [(0, 0, big)], 1, 2), ("size that wraps", 4, [(0, 2, 0)], big - 1, 1),
        ("frame == n_frames", 4, ok + [(4, 0, 0)], 10, 10), ("frame far outside", 4, ok + [(big, 0, 0)], 10, 10),
        ("frames out of order", 4, [(1, 0, 0), (0, 0, 0)], 10, 10), ("frames out of order", 4, ok + [(2, 0, 0)], 10, 10),
    ]
    for what, n_frames, boxes, rows, cols in bad:
        assert boxes_plan(h, w, n_frames, boxes, rows, cols)[0] == -1, what
        assert L.product().ebcc_hip_last_error(), what
    # a geometry the engine refuses, and a keep array with too little room
    assert boxes_plan(0, 10, 1, [(0, 0, 0)], 1, 1)[0] == -1 and boxes_plan(2048, 10, 1, [(0, 0, 0)], 1, 1)[0] == -1
    # a geometry the window decode refuses (j2k_window_supported): fewer than 3 columns; 3 columns are taken
    for width in (1, 2):
        assert boxes_plan(40, width, 1, [(0, 0, 0)], 1, 1)[0] == -1, width           # (boxes_plan checks that keep stays as it was)
        assert b"not supported" in L.product().ebcc_hip_last_error(), width
    n3, keep3 = boxes_plan(40, 3, 2, [(1, 39, 2)], 1, 1)
    assert n3 == len(P.block_list(40, 3)) and keep3[1].any() and not keep3[0].any()
    table = np.zeros((1, 3), np.uint64)
    keep = np.full(4, 0x5A, np.uint8)
    assert _fn()(h, w, 1, table.ctypes.data, 1, 1, 1, keep.ctypes.data, 4) == -1 and (keep == 0x5A).all()


def test_size_overflow_is_refused_before_the_list_is_read():
    """n_boxes * rows * cols beyond SIZE_MAX: the list pointer holds one box, and the call must not get as far as the second"""
    table = np.zeros((1, 3), np.uint64)
    keep = np.full(4, 0x5A, np.uint8)
    for n_boxes, rows, cols in [(1 << 62, 2, 2), (3, 1 << 32, 1 << 32), (1 << 40, 1 << 12, 1 << 12), ((1 << 64) - 1,) * 3]:
        assert _fn()(100, 130, 4, table.ctypes.data, n_boxes, rows, cols, keep.ctypes.data, 4) == -1, (n_boxes, rows, cols)
        assert L.product().ebcc_hip_last_error() and (keep == 0x5A).all(), (n_boxes, rows, cols)
