"""GPU: a window and a box list cut across decode slices (EBCC_HIP_DECODE_SLICES, read per call; the default is one slice, and no
other test sets it together with a window or a box list).  A slice's part of a region - the window from its first frame on, or the
boxes of its frames with their frames counted from it - must put the same bits in the same places as the one-slice decode:
everything is compared bit for bit against crops of the one-slice full decode, through the sentinel harnesses of
tests/test_window_gpu.py and tests/test_box_decode_gpu.py (nothing outside the output may change; after a refusal nothing at all)."""
import ctypes
import os

import numpy as np
import pytest

from tests import _lib as L
from tests import test_box_decode_gpu as B
from tests import test_window_gpu as T

pytestmark = pytest.mark.gpu

H, W = 100, 130
SLICES = "EBCC_HIP_DECODE_SLICES"
same_bits, sha, crop, crops = T.same_bits, T.sha, T.crop, B.crops
WINDOW_ENTRIES = ("ebcc_hip_decode_frames_window", "ebcc_hip_decode_shard_window")
WIN_ODD, WIN_EVEN = (31, 51, 37, 45), (20, 32, 40, 64)                # odd origin and sizes: single stores; all even: pair stores
# the two with a residual layer first; constants go to indices 2 and 5, the legacy form to 6; the sixth golden stream is the ninth
GOLDEN = ["in2_cr30_m2_e0.001_q0.02", "in2_cr5_m1_e0.01_q0.02", "in2_cr10_m0_e0.0_q0.02", "in3_cr30_m1_e0.1_q0.02", "in3_cr100_m1_e2.0_q0.02",
          "in2_cr30_m1_e0.5_q0.02"]
CONSTANTS = {2: 3.25, 5: -1.5}
_batch = []


def batch():
    """nine streams of 100 x 130 and their one-slice full decode, built once: [g0, g1, const 3.25, g2, g3, const -1.5, legacy g0, g4, g5]"""
    if not _batch:
        assert SLICES not in os.environ
        gold = [bytes.fromhex(T.STREAMS[n]["stream_hex"]) for n in GOLDEN]
        assert [T.STREAMS[n]["coeffs_size"] > 0 for n in GOLDEN] == [True, True, False, False, False, False]
        cfg = L.make_config((1, H, W), base_cr=10.0, error=0.01, residual_type=L.MAX_ERROR)
        with L.Context(9, H, W) as ctx:
            const = ctx.encode_frames(np.stack([np.full((H, W), v, np.float32) for v in CONSTANTS.values()]), cfg)
            streams = [gold[0], gold[1], const[0], gold[2], gold[3], const[1], L.legacy_repack(gold[0]), gold[4], gold[5]]
            full = ctx.decode_frames(streams)
        for k, name in ((0, 0), (1, 1), (3, 2), (4, 3), (6, 0), (7, 4), (8, 5)):
            assert sha(full[k].tobytes()) == T.STREAMS[GOLDEN[name]]["decoded_sha256"], (k, GOLDEN[name])
        for k, v in CONSTANTS.items():
            assert (full[k] == np.float32(v)).all(), k
        _batch.append((streams, full))
    return _batch[0]


def host_full(ctx, streams):
    n = len(streams)
    keep, ptrs, sizes = T._args(streams)
    fn = L.product().ebcc_hip_decode_host_frames
    fn.argtypes, fn.restype = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int
    out = np.full(T.PAD_FRONT + n * H * W + T.PAD_BACK, np.float32(-777.25), np.float32)
    assert fn(ctx.ptr, ptrs, sizes, n, out.ctypes.data + 4 * T.PAD_FRONT) == 0, L.product().ebcc_hip_last_error()
    assert (out[:T.PAD_FRONT] == np.float32(-777.25)).all() and (out[T.PAD_FRONT + n * H * W:] == np.float32(-777.25)).all()
    return out[T.PAD_FRONT:T.PAD_FRONT + n * H * W].reshape(n, H, W).copy()


def boxes_21x33():
    """seven boxes on frame 3, five on frame 4 (either side of the cut between two slices of eight frames), two on each constant
    frame, none on frames 1 and 6, a repeated box on frame 7"""
    at = [(0, 0), (79, 97), (40, 50), (13, 64), (64, 13), (33, 1), (1, 33)]
    return ([(0, 5, 7), (0, 70, 90)] + [(2, 0, 0), (2, 60, 31)] + [(3, r, c) for r, c in at] + [(4, r, c) for r, c in at[:5]] +
            [(5, 79, 97), (5, 11, 12)] + [(7, 30, 40), (7, 30, 40), (7, 0, 97)])


def test_one_batch_in_two_slices(monkeypatch):
    """eight frames are the fewest that are cut in two: frames 0 .. 3 and 4 .. 7"""
    streams, full = batch()
    streams, full = streams[:8], full[:8]
    monkeypatch.setenv(SLICES, "2")
    with L.Context(8, H, W) as ctx:
        assert same_bits(ctx.decode_frames(streams), full) and same_bits(ctx.decode_frames(streams, shard=True), full)
        assert same_bits(host_full(ctx, streams), full)
        for win in (WIN_ODD, WIN_EVEN):
            for entry in WINDOW_ENTRIES:
                assert same_bits(T.window(ctx, streams, win, entry), crop(full, win)), (entry, win)
            assert same_bits(T.host_window(ctx, streams, win), crop(full, win)), ("host", win)
        for boxes, rows, cols in ((boxes_21x33(), 21, 33), ([b for b in B.corners(H, W, 8) if b[0] in (0, 3, 4, 7)], 1, 1)):
            want = crops(full, boxes, rows, cols)
            for entry in B.ENTRIES:
                assert same_bits(B.boxes_of(ctx, streams, boxes, rows, cols, entry), want), (entry, rows, cols)
            assert same_bits(B.host_boxes(ctx, streams, boxes, rows, cols), want), ("host", rows, cols)
        assert same_bits(ctx.decode_frames(streams), full)


def test_batches_and_slices_together(monkeypatch):
    """19 streams through a context of 8: two batches of two slices on the two engine sets and a last batch of 3 as one slice"""
    nine, full9 = batch()
    streams = [nine[i % 9] for i in range(19)]
    full = np.stack([full9[i % 9] for i in range(19)])
    monkeypatch.setenv(SLICES, "2")
    # frames 0 .. 7 and 16 .. 18 alone are named: the middle batch's frames are never read
    boxes = [(f, (7 * f) % 80, (11 * f) % 98) for f in range(8)] + [(3, 79, 97), (3, 79, 97), (4, 0, 0)] + [(f, 5 + k, 3 * k) for f in (16, 17, 18) for k in range(3)]
    boxes = sorted(boxes, key=lambda b: b[0])
    absent = [s if f < 8 or f >= 16 else None for f, s in enumerate(streams)]
    with L.Context(8, H, W) as ctx:
        assert same_bits(T.window(ctx, streams, WIN_ODD, WINDOW_ENTRIES[1]), crop(full, WIN_ODD))
        assert same_bits(T.host_window(ctx, streams, WIN_ODD), crop(full, WIN_ODD))
        want = crops(full, boxes, 21, 33)
        assert same_bits(B.boxes_of(ctx, absent, boxes, 21, 33, B.ENTRIES[1]), want)
        assert same_bits(B.host_boxes(ctx, absent, boxes, 21, 33), want)
        assert same_bits(ctx.decode_frames(streams, shard=True), full)


def test_refusals_in_slices_write_nothing(monkeypatch):
    streams, full = batch()
    streams, full = streams[:8], full[:8]
    monkeypatch.setenv(SLICES, "2")
    with L.Context(8, H, W) as ctx:
        for entry in WINDOW_ENTRIES:
            assert T.raw_window(ctx, streams, (99, 129, 2, 1), entry)[0] == 1, entry
            assert L.product().ebcc_hip_last_error(), entry
        for entry in B.ENTRIES:
            assert B.raw_boxes(ctx, streams, [(1, 0, 0), (0, 0, 0)], 10, 10, entry)[0] == 1, entry
            assert L.product().ebcc_hip_last_error(), entry
        assert same_bits(ctx.decode_frames(streams), full)                 # the context still decodes
        assert same_bits(T.window(ctx, streams, WIN_ODD), crop(full, WIN_ODD))


def test_batch_codec_in_slices(monkeypatch):
    from ebcc_amd import h5_batch
    streams, full = batch()
    streams, full = streams[:8], full[:8]
    monkeypatch.setenv(SLICES, "2")
    boxes = np.array(boxes_21x33())
    with h5_batch.BatchCodec(H, W, max_frames=8) as codec:
        assert same_bits(codec.decode(streams), full)
        assert same_bits(codec.decode(streams, window=WIN_ODD), crop(full, WIN_ODD))
        want = crops(full, boxes.tolist(), 21, 33)
        assert same_bits(codec.decode_boxes(streams, boxes, 21, 33), want)
        named = set(boxes[:, 0].tolist())
        assert named == {0, 2, 3, 4, 5, 7}
        assert same_bits(codec.decode_boxes([s if f in named else None for f, s in enumerate(streams)], boxes, 21, 33), want)
