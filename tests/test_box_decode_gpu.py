"""GPU: box-list decode (ebcc_hip_decode_*_boxes, include/ebcc_hip.h): any boxes of any frames in one call.  The criterion is
exact everywhere: box e is, bit for bit (compared as uint32), the crop [row0, row0 + rows) x [col0, col0 + cols) of what
ebcc_hip_decode_frames gives for frame_e on the same context - and that full decode is itself held against the golden hashes
or the oracle.  Device outputs use the harness of tests/test_window_gpu.py: the output lies between sentinel bands at an
address 4 bytes off 8-byte alignment, nothing outside [n_boxes][rows][cols] may change, and after a refusal nothing at all."""
import ctypes
import os
import struct
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest

from tests import _lib as L
from tests import test_window_gpu as T

pytestmark = pytest.mark.gpu

STREAMS = T.STREAMS
SENTINEL, PAD_FRONT, PAD_BACK = T.SENTINEL, T.PAD_FRONT, T.PAD_BACK
same_bits, sha = T.same_bits, T.sha
ENTRIES = ("ebcc_hip_decode_frames_boxes", "ebcc_hip_decode_shard_boxes")
PLACED = ("ebcc_hip_decode_shard_placed", "ebcc_hip_decode_host_frames_placed")


def lib():
    """the product with the box-list entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    sig = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p] + [ctypes.c_size_t] * 3 + [ctypes.c_void_p]
    for name in ENTRIES + ("ebcc_hip_decode_host_frames_boxes",):
        fn = getattr(p, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
    for name in PLACED:
        fn = getattr(p, name)
        fn.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        fn.restype = ctypes.c_int
    return p


def _args(streams):
    """streams: bytes, or None for a frame that is not to be read (NULL, size 0)"""
    n = len(streams)
    bufs = [None if s is None else ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    ptrs = (ctypes.c_void_p * n)(*[None if b is None else ctypes.cast(b, ctypes.c_void_p).value for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in streams])
    return bufs, ptrs, sizes


def _table(boxes):
    return np.ascontiguousarray(np.asarray(boxes, np.uint64).reshape(-1, 3))          # == ebcc_hip_box[]


def raw_boxes(ctx, streams, boxes, rows, cols, entry=ENTRIES[0], n_frames=None):
    """-> (return value, [k][rows][cols] or None); asserts that nothing outside the output was written, and after a non-zero
    return nothing at all"""
    n = len(streams) if n_frames is None else n_frames
    keep, ptrs, sizes = _args(streams)
    table = _table(boxes)
    k = len(table)
    count = k * rows * cols if 0 < rows * cols < (1 << 40) else 0
    total = PAD_FRONT + count + PAD_BACK
    host = np.full(total * 4, SENTINEL, np.uint8)
    d = L.DeviceArray(host)
    rc = getattr(lib(), entry)(ctx.ptr, ptrs, sizes, n, table.ctypes.data if k else None, k, rows, cols, d.ptr + 4 * PAD_FRONT)
    back = d.get(np.uint8, (total * 4,))
    d.free()
    assert (back[:4 * PAD_FRONT] == SENTINEL).all() and (back[4 * (PAD_FRONT + count):] == SENTINEL).all(), ("written outside the output", rows, cols)
    if rc:
        assert (back == SENTINEL).all(), ("written by a call that failed", rows, cols)
        return rc, None
    return rc, back[4 * PAD_FRONT:4 * (PAD_FRONT + count)].view(np.float32).reshape(k, rows, cols).copy()


def boxes_of(ctx, streams, boxes, rows, cols, entry=ENTRIES[0]):
    rc, out = raw_boxes(ctx, streams, boxes, rows, cols, entry)
    assert rc == 0, (rows, cols, L.product().ebcc_hip_last_error())
    return out


def host_boxes(ctx, streams, boxes, rows, cols):
    keep, ptrs, sizes = _args(streams)
    table = _table(boxes)
    k = len(table)
    out = np.full(PAD_FRONT + k * rows * cols + PAD_BACK, np.float32(-777.25), np.float32)
    rc = lib().ebcc_hip_decode_host_frames_boxes(ctx.ptr, ptrs, sizes, len(streams), table.ctypes.data, k, rows, cols, out.ctypes.data + 4 * PAD_FRONT)
    assert rc == 0, (rows, cols, L.product().ebcc_hip_last_error())
    assert (out[:PAD_FRONT] == np.float32(-777.25)).all() and (out[PAD_FRONT + k * rows * cols:] == np.float32(-777.25)).all()
    return out[PAD_FRONT:PAD_FRONT + k * rows * cols].reshape(k, rows, cols).copy()


def crops(full, boxes, rows, cols):
    return np.stack([full[f, r0:r0 + rows, c0:c0 + cols] for f, r0, c0 in boxes])


def check(ctx, streams, full, boxes, rows, cols, entry=ENTRIES[0], what=None):
    boxes = sorted(boxes, key=lambda b: b[0])                            # (stable: the order within a frame stays)
    got = boxes_of(ctx, streams, boxes, rows, cols, entry)
    want = crops(full, boxes, rows, cols)
    bad = [e for e in range(len(boxes)) if not same_bits(got[e], want[e])]
    assert not bad, (what, rows, cols, entry, [boxes[e] for e in bad[:5]], len(bad))
    return got


# ---- box lists -----------------------------------------------------------------------------------------------------------------
def windows_as_lists(h, w, n_frames, n_random=40):
    """the catalogue and the random windows of tests/test_window_plan.py (as tests/test_window_gpu.py draws them), regrouped by
    size - all boxes of a call have one size - and every window put on three of the frames"""
    rng = np.random.default_rng(17 * h + w)
    groups = defaultdict(list)
    for r0, c0, rows, cols in T.windows_of(h, w, n_random):
        for f in rng.choice(n_frames, size=min(3, n_frames), replace=False):
            groups[(rows, cols)].append((int(f), r0, c0))
    return sorted(groups.items())


def moving(h, w, n_frames, rows, cols, dr, dc):
    return [(f, (f * dr) % (h - rows + 1), (f * dc) % (w - cols + 1)) for f in range(n_frames)]


def twelve_per_frame(h, w, n_frames, rows=16, cols=20):
    """identical, overlapping and abutting boxes, at the edges and across the code-block boundary at 64"""
    at = [(0, 0), (0, 0), (3, 5), (3, 5 + cols), (3 + rows, 5), (h - rows, w - cols), (h - rows, 0), (0, w - cols), (64 - rows // 2, 64 - cols // 2),
          (64 - rows, 64 - cols), (64, 64), (h // 2, w // 3)]
    return [(f, min(r, h - rows), min(c, w - cols)) for f in range(n_frames) for r, c in at]


def corners(h, w, n_frames):
    return [(f, r, c) for f in range(n_frames) for r, c in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))]


def random_boxes(h, w, n_frames, rows, cols, k, seed):
    rng = np.random.default_rng(seed)
    return sorted([(int(rng.integers(0, n_frames)), int(rng.integers(0, h - rows + 1)), int(rng.integers(0, w - cols + 1))) for _ in range(k)],
                  key=lambda b: b[0])


# ---- 1. golden mixed batches ---------------------------------------------------------------------------------------------------
def golden_batch(h, w):
    """every single-frame stream of codec_streams.json of the shape and its header-less form: (names, streams)"""
    names = [n for n, c in sorted(STREAMS.items()) if (c["h"], c["w"]) == (h, w)]
    streams = [bytes.fromhex(STREAMS[n]["stream_hex"]) for n in names]
    return names, streams + [L.legacy_repack(s) for s in streams]


def golden_full(ctx, names, streams):
    full = ctx.decode_frames(streams)
    for k, n in enumerate(names):
        assert sha(full[k].tobytes()) == STREAMS[n]["decoded_sha256"] == sha(full[len(names) + k].tobytes()), n
    return full


def golden_case(h, w, n_random=40):
    names, streams = golden_batch(h, w)
    n = len(streams)
    with L.Context(n, h, w) as ctx:
        full = golden_full(ctx, names, streams)
        for (rows, cols), boxes in windows_as_lists(h, w, n, n_random):
            check(ctx, streams, full, boxes, rows, cols, what="catalogue")
        check(ctx, streams, full, moving(h, w, n, 17, 23, 5, 7), 17, 23, what="moving origin")
        check(ctx, streams, full, twelve_per_frame(h, w, n), 16, 20, what="12 boxes a frame")
        check(ctx, streams, full, corners(h, w, n), 1, 1, what="corners")
        check(ctx, streams, full, [(f, 0, 0) for f in range(n)], h, w, what="whole frame")
        assert same_bits(ctx.decode_frames(streams), full)


@pytest.mark.parametrize("h,w", [(64, 96), (100, 130)])
def test_golden_mixed_batches(h, w):
    """the three modes, the constant field, kept residuals, legacy forms: one mixed batch per shape"""
    golden_case(h, w)


# ---- 2. product-coded frames ---------------------------------------------------------------------------------------------------
MODES = [(L.MAX_ERROR, 0.5), (L.RELATIVE_ERROR, 1e-3)]
_coded = {}


def coded(h, w, n, mode, err, base_cr=10.0):
    """n era5_like frames of h x w coded by the product: (streams, the oracle's decode of them)"""
    key = (h, w, n, mode)
    if key not in _coded:
        frames = np.stack([L.era5_like(h, w, s, 1.2 + 0.1 * (s % 5), 1.0 + 0.5 * (s % 4)) for s in range(n)])
        cfg = L.make_config((1, h, w), base_cr=base_cr, error=err, residual_type=mode)
        with L.Context(n, h, w) as ctx:
            streams = ctx.encode_frames(frames, cfg)
        _coded[key] = (streams, T.oracle_fields(streams, h, w))
    return _coded[key]


def product_full(ctx, streams, ref):
    full = ctx.decode_frames(streams)
    assert np.array_equal(full, ref), "full decode differs from the oracle"
    return full


@pytest.mark.parametrize("mode,err", MODES, ids=["abs", "rel"])
def test_odd_frames_97x131(mode, err):
    """odd both ways: single stores everywhere and the last, odd column"""
    h, w, n = 97, 131, 4
    streams, ref = coded(h, w, n, mode, err)
    with L.Context(n, h, w) as ctx:
        full = product_full(ctx, streams, ref)
        check(ctx, streams, full, [(f, 0, w - 1) for f in range(n)], h, 1, what="last column")
        check(ctx, streams, full, [(f, h - 1, 0) for f in range(n)], 1, w, what="last row")
        check(ctx, streams, full, twelve_per_frame(h, w, n, 15, 21), 15, 21)
        check(ctx, streams, full, twelve_per_frame(h, w, n, 16, 20), 16, 20)
        check(ctx, streams, full, random_boxes(h, w, n, 33, 41, 23, 5), 33, 41)
        check(ctx, streams, full, corners(h, w, n), 1, 1)
        check(ctx, streams, full, [(f, 0, 0) for f in range(n)], h, w)


@pytest.mark.parametrize("mode,err", MODES, ids=["abs", "rel"])
def test_level_1_unfused_40x32(mode, err):
    """width 32: level 1 takes the separate passes and leaves the frame's band in the frames' buffer, which every box of the
    frame, in every round (27 and 48 boxes through 4 slots), reads"""
    h, w, n = 40, 32, 4
    streams, ref = coded(h, w, n, mode, err)
    with L.Context(n, h, w) as ctx:
        full = product_full(ctx, streams, ref)
        check(ctx, streams, full, random_boxes(h, w, n, 9, 11, 27, 1), 9, 11)
        check(ctx, streams, full, twelve_per_frame(h, w, n, 8, 6), 8, 6)
        check(ctx, streams, full, corners(h, w, n), 1, 1)
        check(ctx, streams, full, [(f, 0, 0) for f in range(n)] * 2, h, w)
        assert same_bits(ctx.decode_frames(streams), full)


@pytest.mark.parametrize("mode,err", MODES, ids=["abs", "rel"])
def test_strips_and_pieces_160x520(mode, err):
    """five top-level strips (two workgroups at four waves each), entries of one launch with differing strip counts, cones of
    64 rows and more (several pieces)"""
    h, w, n = 160, 520, 3
    streams, ref = coded(h, w, n, mode, err)
    with L.Context(n, h, w) as ctx:
        full = product_full(ctx, streams, ref)
        # 100 columns are 50 pairs of the top level: one strip of 60 pairs or two, by position; 130 columns are two or three
        check(ctx, streams, full, [(f, r0, c0) for f in range(n) for r0, c0 in ((0, 10), (60, 100), (90, 236), (45, 420), (7, 300))], 70, 100, what="1-2 strips")
        check(ctx, streams, full, [(f, r0, c0) for f in range(n) for r0, c0 in ((0, 0), (30, 110), (60, 118), (11, 390), (25, 238))], 100, 130, what="2-3 strips")
        # 236 columns: 2 or 3 strips of the top level, and at level 4 one strip at the left edge (the cone ends at sample 120)
        # and two anywhere else
        check(ctx, streams, full, [(f, r0, c0) for f in range(n) for r0, c0 in ((0, 0), (20, 2), (90, 119), (60, 284), (33, 241))], 70, 236, what="1-3 strips")
        check(ctx, streams, full, [(f, r0, 0) for f in range(n) for r0 in (0, 96, 33)], 64, w, what="5 strips")
        check(ctx, streams, full, [(f, 0, 0) for f in range(n)], h, w, what="whole frame")
        check(ctx, streams, full, random_boxes(h, w, n, 1, 1, 40, 9), 1, 1, what="points")


# ---- 3. rounds ------------------------------------------------------------------------------------------------------------------
def rounds_case():
    """5 frames of 100 x 130, 60 boxes: twelve a frame - through 5 slots every frame is named in three rounds and its boxes are
    split across the round boundaries - and through 16 slots; same bits from both"""
    h, w = 100, 130
    names = [n for n, c in sorted(STREAMS.items()) if (c["h"], c["w"]) == (h, w)][:5]
    streams = [bytes.fromhex(STREAMS[n]["stream_hex"]) for n in names]
    boxes = sorted(random_boxes(h, w, 5, 21, 33, 40, 4) + [(f, r, c) for f in range(5) for r, c in ((0, 0), (79, 97), (40, 50), (40, 50))], key=lambda b: b[0])
    assert len(boxes) == 60
    got = []
    for cap in (5, 16):
        with L.Context(cap, h, w) as ctx:
            full = ctx.decode_frames(streams)
            for n, d in zip(names, full):
                assert sha(d.tobytes()) == STREAMS[n]["decoded_sha256"], n
            got.append(check(ctx, streams, full, boxes, 21, 33, what=f"capacity {cap}"))
            check(ctx, streams, full, [b for b in boxes if b[0] in (0, 4)], 21, 33, what="two frames, many rounds")
    assert same_bits(got[0], got[1])


def test_rounds():
    rounds_case()


# ---- 4. unnamed frames ----------------------------------------------------------------------------------------------------------
def five_of_100x130(mode=L.MAX_ERROR):
    names = [n for n, c in sorted(STREAMS.items()) if (c["h"], c["w"]) == (100, 130) and c["mode"] == mode][:5]
    assert len(names) == 5
    return [bytes.fromhex(STREAMS[n]["stream_hex"]) for n in names]


def test_unnamed_frames_are_not_read():
    streams = five_of_100x130()
    boxes = [(1, 10, 20), (1, 50, 60), (3, 0, 0), (3, 70, 100), (3, 70, 100)]
    with L.Context(5, 100, 130) as ctx:
        full = ctx.decode_frames(streams)
        want = check(ctx, streams, full, boxes, 30, 30)
        for entry in ENTRIES:
            absent = [s if f in (1, 3) else None for f, s in enumerate(streams)]
            assert same_bits(boxes_of(ctx, absent, boxes, 30, 30, entry), want), entry
            garbage = [s if f in (1, 3) else bytes((37 * i + f) & 0xFF for i in range(300)) for f, s in enumerate(streams)]
            assert same_bits(boxes_of(ctx, garbage, boxes, 30, 30, entry), want), entry
        assert same_bits(host_boxes(ctx, absent, boxes, 30, 30), want)


def test_truncated_stream_of_a_named_frame_is_refused_like_the_full_decode():
    streams = five_of_100x130()[:4]
    s = streams[2]
    tail = struct.unpack("<Q", s[40:48])[0]
    cut = 40
    assert tail > 200
    bad = list(streams)
    bad[2] = s[:40] + struct.pack("<Q", tail - cut) + s[48:len(s) - cut]               # a consistent header over a codestream that ends early
    with L.Context(4, 100, 130) as ctx:
        keep, ptrs, sizes = _args(bad)
        out = L.DeviceArray(nbytes=4 * 100 * 130 * 4)
        assert L.product().ebcc_hip_decode_frames(ctx.ptr, ptrs, sizes, 4, out.ptr) != 0
        out.free()
        for entry in ENTRIES:
            rc, _ = raw_boxes(ctx, bad, [(0, 0, 0), (2, 10, 10)], 30, 30, entry)
            assert rc != 0, entry
            assert raw_boxes(ctx, bad, [(0, 0, 0), (3, 10, 10)], 30, 30, entry)[0] == 0, entry      # (the bad frame is not named)
        full = ctx.decode_frames(streams)
        check(ctx, streams, full, [(0, 0, 0), (2, 10, 10)], 30, 30)


# ---- 5. refusals: return value 1, a message, nothing written (raw_boxes checks the whole buffer) ---------------------------
def test_refusals_write_nothing():
    streams = five_of_100x130()
    big = (1 << 64) - 1
    ok = [(0, 0, 0), (1, 5, 5), (4, 90, 120)]
    cases = [("no boxes", [], 10, 10), ("rows zero", ok, 0, 10), ("cols zero", ok, 10, 0),
             ("below the frame", ok + [(4, 91, 0)], 10, 10), ("right of the frame", ok + [(4, 0, 121)], 10, 10),
             ("taller than the frame", [(0, 0, 0)], 101, 1), ("wider than the frame", [(0, 0, 0)], 1, 131),
             ("origin that wraps", [(0, big, 0)], 2, 1), ("origin that wraps", [(0, 0, big)], 1, 2), ("size that wraps", [(0, 2, 0)], big - 1, 1),
             ("frame == n_frames", ok + [(5, 0, 0)], 10, 10), ("frame far outside", ok + [(big, 0, 0)], 10, 10),
             ("frames out of order", [(1, 0, 0), (0, 0, 0)], 10, 10), ("frames out of order", ok + [(3, 0, 0)], 10, 10)]
    with L.Context(5, 100, 130) as ctx:
        for entry in ENTRIES:
            for what, boxes, rows, cols in cases:
                rc, _ = raw_boxes(ctx, streams, boxes, rows, cols, entry)
                assert rc == 1, (entry, what)
                assert L.product().ebcc_hip_last_error(), (entry, what)
        keep, ptrs, sizes = _args(streams)
        out = np.full(64, np.float32(3.5), np.float32)
        table = _table([(0, 99, 0)])
        assert lib().ebcc_hip_decode_host_frames_boxes(ctx.ptr, ptrs, sizes, 5, table.ctypes.data, 1, 2, 1, out.ctypes.data) == 1
        assert (out == np.float32(3.5)).all()
        full = ctx.decode_frames(streams)                                 # the context still works
        check(ctx, streams, full, [(4, 99, 129)], 1, 1)
    with L.Context(3, 100, 130) as ctx:                                   # more frames than the context holds: the one-batch form refuses
        assert raw_boxes(ctx, streams, ok, 10, 10, ENTRIES[0])[0] == 1
        assert raw_boxes(ctx, streams, ok, 10, 10, ENTRIES[1])[0] == 0


# ---- 6. shard and host forms ---------------------------------------------------------------------------------------------------
def test_shard_and_host_forms():
    """8 frames through a context of 3: several batches on the two engine sets, every batch a contiguous part of the output;
    lists that leave frames - whole batches of them - without a box, give one box to a frame and many to another"""
    h, w = 100, 130
    names = [n for n, c in sorted(STREAMS.items()) if (c["h"], c["w"]) == (h, w)][:8]
    streams = [bytes.fromhex(STREAMS[n]["stream_hex"]) for n in names]
    lists = [[(f, (7 * f) % 60, (11 * f) % 90) for f in range(8)],                                          # one a frame
             [(0, 1, 1), (1, 2, 2), (2, 3, 3), (7, 4, 4)] + [(7, 5 + k, 3 * k) for k in range(20)],             # frames 3 .. 6 without a box
             [(4, 50, 60)],                                                                                   # one box in all
             random_boxes(h, w, 8, 40, 40, 50, 2)]
    with L.Context(3, h, w) as ctx:
        full = ctx.decode_frames(streams, shard=True)
        for n, d in zip(names, full):
            assert sha(d.tobytes()) == STREAMS[n]["decoded_sha256"], n
        for boxes in lists:
            boxes = sorted(boxes, key=lambda b: b[0])
            want = crops(full, boxes, 40, 40)
            assert same_bits(boxes_of(ctx, streams, boxes, 40, 40, ENTRIES[1]), want), ("shard", boxes[:3])
            assert same_bits(host_boxes(ctx, streams, boxes, 40, 40), want), ("host", boxes[:3])
        assert same_bits(ctx.decode_frames(streams, shard=True), full)


# ---- 7. full-size frames, once -------------------------------------------------------------------------------------------------
def test_full_size_frames():
    h, w, n = 721, 1440, 6
    streams, ref = coded(h, w, n, L.MAX_ERROR, 0.5, base_cr=30.0)
    rng = np.random.default_rng(8)
    with L.Context(n, h, w) as ctx:
        full = product_full(ctx, streams, ref)
        for k, (r0, c0, rows, cols) in enumerate(T.ENTRY_WINDOWS):       # every window of that list on two frames that differ from its neighbours'
            check(ctx, streams, full, [(k % n, r0, c0), ((k + 3) % n, r0, c0)], rows, cols, what="entry windows")
        check(ctx, streams, full, [(f, 300 + 10 * f, 100 + 40 * f) for f in range(n)], 128, 256, what="moving box")
        check(ctx, streams, full, random_boxes(h, w, n, 32, 32, 40, 12), 32, 32, what="crops")     # (seven rounds of six slots)
        pts = [(int(f), int(rng.integers(0, h)), int(rng.integers(0, w))) for f in range(n) for _ in range(3)]
        check(ctx, streams, full, pts, 1, 1, what="points")
        assert same_bits(ctx.decode_frames(streams), full)


# ---- 8. poisoned workspace: slots and tables are not read before they are written ------------------------------------------
def _poisoned_child():
    golden_case(100, 130, 12)
    rounds_case()
    print("BOX_CHILD ok", flush=True)


@pytest.mark.parametrize("pattern", ["0xFF", "0x7F"])
def test_poisoned_workspace(pattern):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EBCC_")}
    env["EBCC_HIP_POISON_ALLOC"] = pattern
    code = f"import sys; sys.path.insert(0, {L.ROOT!r}); from tests import test_box_decode_gpu as B; B._poisoned_child()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=L.ROOT, timeout=600)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-1500:]}{r.stderr[-3000:]}"
    assert "BOX_CHILD ok" in r.stdout


# ---- 9. BatchCodec.decode_boxes -------------------------------------------------------------------------------------------------
def test_batch_codec_decode_boxes():
    from ebcc_amd import h5_batch
    h, w = 100, 130
    streams = five_of_100x130() + five_of_100x130(L.RELATIVE_ERROR)[:3]
    boxes = np.array(random_boxes(h, w, len(streams), 24, 40, 30, 6))
    with h5_batch.BatchCodec(h, w, max_frames=3) as codec:
        full = codec.decode(streams)
        got = codec.decode_boxes(streams, boxes, 24, 40)
        assert got.shape == (30, 24, 40) and got.dtype == np.float32 and same_bits(got, crops(full, boxes.tolist(), 24, 40))
        into = np.full((30, 24, 40), -1.0, np.float32)
        assert codec.decode_boxes(streams, boxes, 24, 40, out=into) is into and same_bits(into, got)
        named = set(boxes[:, 0].tolist())
        assert same_bits(codec.decode_boxes([s if f in named else None for f, s in enumerate(streams)], boxes, 24, 40), got)
        for bad, rows, cols in [(boxes[::-1], 24, 40), (boxes, 0, 40), (boxes, 24, 131), (np.array([[0, 77, 0]]), 24, 40), (np.array([[8, 0, 0]]), 24, 40),
                                (np.array([[0, -1, 0]]), 24, 40), (np.zeros((0, 3), np.int64), 24, 40), (np.zeros((2, 2), np.int64), 24, 40)]:
            with pytest.raises(ValueError):
                codec.decode_boxes(streams, bad, rows, cols)
        assert same_bits(codec.decode(streams), full)


# ---- 10. read_boxes / read_points ----------------------------------------------------------------------------------------------
def test_read_boxes_and_points(tmp_path):
    """h5_batch.read_boxes / read_points under an interpreter with h5py, as tests/test_window_gpu.py drives read_frames(rows, cols)"""
    if not os.path.exists(T.CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([T.CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([T.CONDA_PY, os.path.join(L.ROOT, "tests", "h5_box_read.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 3, r.stdout


# ---- 11. a box list is the placed list of a compact array: shard and host forms of both, three batches ----------------------
SEVEN_CONST, SEVEN_BASE_ONLY = 4, 1
FOUR_FORMS = (ENTRIES[1], "ebcc_hip_decode_host_frames_boxes") + PLACED
GUARD = np.uint32(0xA5A5A5A5)
_seven = []


def seven_of_100x130():
    """7 frames of 100 x 130 coded by the product - frame 4 a constant field, frame 1 without a residual layer, the others with
    one: era5_like seeds that keep theirs at base_cr 5, MAX_ERROR 0.01 under a loose base layer - and what
    ebcc_hip_decode_frames gives for them on a context of capacity 3: (streams, full), made once"""
    if not _seven:
        h, w, n = 100, 130, 7
        frames = np.stack([L.era5_like(h, w, s) for s in (9, 13, 14, 15, 0, 16, 13)])
        frames[SEVEN_CONST] = np.float32(281.5)
        before = os.environ.get("EBCC_INIT_BASE_ERROR_QUANTILE")
        os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = "0.1"
        try:
            with L.Context(n, h, w) as ctx:
                streams = ctx.encode_frames(frames, L.make_config((1, h, w), base_cr=5.0, error=0.01, residual_type=L.MAX_ERROR))
                streams[SEVEN_BASE_ONLY] = ctx.encode_frames(frames[SEVEN_BASE_ONLY:SEVEN_BASE_ONLY + 1],
                                                             L.make_config((1, h, w), base_cr=10.0, error=0.0, residual_type=L.NONE))[0]
        finally:
            if before is None:
                del os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"]
            else:
                os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = before
        for f, st in enumerate(streams):
            flags, coeffs, zsize = st[5], struct.unpack("<Q", st[16:24])[0], struct.unpack("<Q", st[32:40])[0]
            assert st[:4] == b"EBCC" and bool(flags & 1) == (f == SEVEN_CONST), f
            assert (coeffs > 0 and zsize > 0) == (f not in (SEVEN_CONST, SEVEN_BASE_ONLY)), (f, coeffs, zsize)     # a residual layer
        with L.Context(3, h, w) as ctx:
            full = np.concatenate([ctx.decode_frames(streams[lo:lo + 3]) for lo in range(0, n, 3)])
        assert (full[SEVEN_CONST] == np.float32(281.5)).all()
        full.setflags(write=False)
        _seven.append((streams, full))
    return _seven[0]


def guarded(ctx, streams, form, boxes, rows, cols, front, n_frames=None):
    """the box list through a _boxes form, or the equal placed list - box e of rows x cols at offset e * rows * cols, pitch cols -
    through a _placed form, into k * rows * cols floats that begin `front` floats behind an 8-byte aligned address, between
    guard words, on the device or (host forms) in host memory -> (return value, the output's words as uint32); asserts that
    the guards are intact, and after a non-zero return the whole array"""
    n = len(streams) if n_frames is None else n_frames
    keep, ptrs, sizes = _args(streams)
    k, count = len(boxes), len(boxes) * rows * cols
    words = np.full(front + count + PAD_BACK, GUARD, np.uint32)
    fn = getattr(lib(), form)
    if form in PLACED:
        table = np.array([(f, r0, c0, rows, cols, e * rows * cols, cols) for e, (f, r0, c0) in enumerate(boxes)], np.uint64)   # == ebcc_hip_placed_box[]
        call = lambda out: fn(ctx.ptr, ptrs, sizes, n, table.ctypes.data, k, out, count)
    else:
        table = _table(boxes)
        call = lambda out: fn(ctx.ptr, ptrs, sizes, n, table.ctypes.data, k, rows, cols, out)
    if "host" in form:
        assert words.ctypes.data % 8 == 0
        rc, back = call(words.ctypes.data + 4 * front), words
    else:
        d = L.DeviceArray(words)
        assert d.ptr % 8 == 0
        rc = call(d.ptr + 4 * front)
        back = d.get(np.uint32, words.shape)
        d.free()
    assert (back[:front] == GUARD).all() and (back[front + count:] == GUARD).all(), ("written outside the output", form)
    if rc:
        assert (back == GUARD).all(), ("written by a call that failed", form)
    return rc, back[front:front + count].copy()


def four_forms(ctx, streams, full, boxes, rows, cols, front, what):
    """all four forms give the crops, bit for bit -> the output [k][rows][cols]"""
    want = np.ascontiguousarray(crops(full, boxes, rows, cols)).view(np.uint32).ravel()
    for form in FOUR_FORMS:
        rc, got = guarded(ctx, streams, form, boxes, rows, cols, front)
        assert rc == 0, (what, form, L.product().ebcc_hip_last_error())
        assert np.array_equal(got, want), (what, form, rows, cols, int((got != want).sum()))
    return want.view(np.float32).reshape(len(boxes), rows, cols)


@pytest.mark.parametrize("rows,cols,front", [(5, 7, 1), (6, 8, 2)], ids=["5x7-unaligned", "6x8-pairs"])
def test_boxes_equal_their_placed_list(rows, cols, front):
    """four boxes a frame - a repeat among them, odd and even first columns, the last rows and columns - of every frame, the
    constant one included: twelve boxes a batch through three slots.  5 x 7: 35 floats a box, so the first samples alternate
    between 8-byte aligned and not; 6 x 8 in an 8-byte aligned output: the pair stores"""
    h, w = 100, 130
    streams, full = seven_of_100x130()
    boxes = [b for f in range(7) for b in ((f, (7 * f) % (h - rows), (11 * f) % (w - cols)), (f, 40, 60), (f, 40, 60), (f, h - rows, w - cols))]
    with L.Context(3, h, w) as ctx:
        four_forms(ctx, streams, full, boxes, rows, cols, front, "equality")


def test_constant_frames_across_rounds_and_batches():
    """the constant frame's boxes in the second round of the second batch (every frame named, four boxes on the frame before
    it), in the second round of the first batch (frames 2 .. 6 named) and on both sides of a round boundary"""
    h, w, rows, cols, c = 100, 130, 9, 11, SEVEN_CONST
    streams, full = seven_of_100x130()
    spread = lambda f, k: [(f, (13 * f + 29 * j) % (h - rows), (17 * f + 31 * j) % (w - cols)) for j in range(k)]
    lists = {"second batch, second round": [b for f in range(7) for b in spread(f, 4 if f == c - 1 else 2)],
             "first batch, second round": [b for f in range(2, 7) for b in spread(f, 2)],
             "across a round boundary": [b for f in range(7) for b in spread(f, 4 if f == c else 1)]}
    with L.Context(3, h, w) as ctx:
        for what, boxes in lists.items():
            got = four_forms(ctx, streams, full, boxes, rows, cols, 1, what)
            const = np.array([f == c for f, _, _ in boxes])
            assert const.sum() >= 2 and (got[const] == np.float32(281.5)).all(), what
            assert not (got[~const] == np.float32(281.5)).any(), what


def test_host_form_writes_nothing_else():
    h, w = 100, 130
    streams, full = seven_of_100x130()
    boxes = [(f, 10 * f, 15 * f) for f in range(7)]
    with L.Context(3, h, w) as ctx:
        for form in ("ebcc_hip_decode_host_frames_boxes", PLACED[1]):
            rc, got = guarded(ctx, streams, form, boxes, 20, 30, 3)                  # (guarded: the guards before and behind)
            assert rc == 0 and np.array_equal(got, np.ascontiguousarray(crops(full, boxes, 20, 30)).view(np.uint32).ravel()), form
            rc, _ = guarded(ctx, streams, form, boxes[:6] + [(7, 0, 0)], 20, 30, 3)      # (guarded: the whole array)
            assert rc == 1 and L.product().ebcc_hip_last_error(), form


def test_size_overflow_is_refused_before_the_list_is_read():
    """n_boxes * rows * cols beyond SIZE_MAX: the list pointer holds one box, and the call must not get as far as the second"""
    streams, _ = seven_of_100x130()
    keep, ptrs, sizes = _args(streams)
    table = np.zeros((1, 3), np.uint64)
    words = np.full(64, GUARD, np.uint32)
    with L.Context(3, 100, 130) as ctx:
        for n_boxes, rows, cols in [(1 << 62, 2, 2), (3, 1 << 32, 1 << 32), (1 << 40, 1 << 12, 1 << 12), ((1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 1)]:
            for form in ENTRIES[1:] + ("ebcc_hip_decode_host_frames_boxes",):
                d = L.DeviceArray(words)
                out = words.ctypes.data if "host" in form else d.ptr
                assert getattr(lib(), form)(ctx.ptr, ptrs, sizes, 7, table.ctypes.data, n_boxes, rows, cols, out) == 1, (form, n_boxes, rows, cols)
                assert L.product().ebcc_hip_last_error(), (form, n_boxes, rows, cols)
                assert (words == GUARD).all() and (d.get(np.uint32, words.shape) == GUARD).all(), form
                d.free()
