"""GPU: placed boxes (ebcc_hip_decode_*_placed) and slabs of a chunk container (ebcc_hip_decode_container_slab*,
ebcc_decode_chunking_slab, include/ebcc_hip.h).  Every comparison is bitwise (uint32), with no tolerance: a placed box is the
crop of what ebcc_hip_decode_frames gives on the same context, a slab is the slice of what ebcc_decode_chunking gives for the
same container - and the existing suite holds both of those against the reference build.  Outputs are pre-filled with a
sentinel bit pattern: inside a box's rectangle the output is the crop, every other byte - the gaps between the rectangles, the
pitch's slack, what lies before and behind - is unchanged, and after a refusal all of it is."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from ebcc_amd import sharding
from tests import _lib as L
from tests import test_box_decode_gpu as B
from tests import test_codec_gpu as C

pytestmark = pytest.mark.gpu

same_bits = B.same_bits
SENT = np.uint32(0xA5A5A5A5)
FRONT, BACK = 64, 37                                  # floats of sentinel before (256 bytes: the base offset counts from a 256-byte boundary) and behind
FORMS = ("ebcc_hip_decode_frames_placed", "ebcc_hip_decode_shard_placed", "ebcc_hip_decode_host_frames_placed")


class Slab(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in ("t0", "row0", "col0", "nt", "rows", "cols")]


def lib():
    """the product with the new entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    for name in FORMS:
        fn = getattr(p, name)
        fn.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        fn.restype = ctypes.c_int
    for name in ("ebcc_hip_decode_container_slab", "ebcc_hip_decode_container_slab_host"):
        fn = getattr(p, name)
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    fn = getattr(p, "ebcc_decode_chunking_slab")
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, L.c_void_pp], ctypes.c_size_t
    return p


def error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


# ---- placed boxes ---------------------------------------------------------------------------------------------------------------
def laid_out(boxes, extra=0, gap=5):
    """(frame, row0, col0, rows, cols) in frame order -> ((k, 7) table with each box behind the last at pitch cols + extra and
    `gap` floats between them, floats of the output)"""
    table, at = [], 0
    for f, r0, c0, rows, cols in boxes:
        table.append((f, r0, c0, rows, cols, at, cols + extra))
        at += (rows - 1) * (cols + extra) + cols + gap
    return np.array(table, np.int64), at - gap


def raw_placed(ctx, streams, table, out_floats, form=FORMS[0], base=1, n_frames=None):
    """-> (return value, the output's out_floats uint32 words); the output begins `base` floats behind a 256-byte boundary of a
    sentinel-filled buffer; asserts that nothing before or behind it was written, and after a non-zero return nothing at all"""
    n = len(streams) if n_frames is None else n_frames
    keep, ptrs, sizes = B._args(streams)
    t = np.ascontiguousarray(np.asarray(table, np.uint64).reshape(-1, 7))              # == ebcc_hip_placed_box[]
    room = min(out_floats, 1 << 24)
    words = np.full(FRONT + base + room + BACK, SENT, np.uint32)
    fn = getattr(lib(), form)
    if "host" in form:
        rc = fn(ctx.ptr, ptrs, sizes, n, t.ctypes.data if len(t) else None, len(t), words.ctypes.data + 4 * (FRONT + base), out_floats)
        back = words
    else:
        d = L.DeviceArray(words)
        assert d.ptr % 256 == 0
        rc = fn(ctx.ptr, ptrs, sizes, n, t.ctypes.data if len(t) else None, len(t), d.ptr + 4 * (FRONT + base), out_floats)
        back = d.get(np.uint32, words.shape)
        d.free()
    assert (back[:FRONT + base] == SENT).all() and (back[FRONT + base + room:] == SENT).all(), ("written outside the output", form)
    if rc:
        assert (back == SENT).all(), ("written by a call that failed", form)
    return rc, back[FRONT + base:FRONT + base + room].copy()


def expected(full, table, out_floats):
    want = np.full(out_floats, SENT, np.uint32)
    for f, r0, c0, rows, cols, at, pitch in np.asarray(table).tolist():
        where = at + np.arange(rows)[:, None] * pitch + np.arange(cols)[None, :]
        want[where] = np.ascontiguousarray(full[f, r0:r0 + rows, c0:c0 + cols]).view(np.uint32)
    return want


def check_placed(ctx, streams, full, boxes, extra=0, form=FORMS[0], base=1, what=None):
    table, floats = laid_out(sorted(boxes, key=lambda b: b[0]), extra)
    rc, got = raw_placed(ctx, streams, table, floats, form, base)
    assert rc == 0, (what, form, error())
    want = expected(full, table, floats)
    assert np.array_equal(got, want), (what, form, extra, base, int((got != want).sum()))
    return got


def mixed_boxes(h, w, frames):
    """boxes of different sizes in one call: 1 x 1, 1 x W, H x 1, H x W, 17 x 23, odd and even col0 / cols"""
    out = []
    for f in frames:
        out += [(f, 0, 0, 1, 1), (f, h - 1, w - 1, 1, 1), (f, h // 2, 0, 1, w), (f, 0, w // 3, h, 1), (f, 0, 0, h, w),
                (f, min(3, h - 17), min(5, w - 23), 17, 23), (f, h - 17, (w - 23) & ~1, 17, 23), (f, 2, 4, 16, 20), (f, 1, 7, 10, 12),
                (f, h - 9, w - 13, 9, 12)]
    return out


def all_forms(ctx, streams, full, boxes, what):
    """pitches cols, cols + 1, cols + 3 and bases 0 .. 3 floats behind a 256-byte boundary on the device form; each once more on
    the shard and the host form"""
    for extra in (0, 1, 3):
        for base in (0, 1, 2, 3):
            check_placed(ctx, streams, full, boxes, extra, FORMS[0], base, what)
    for k, form in enumerate(FORMS[1:]):
        for extra, base in ((0, k), (1, 2 + k), (3, 1)):
            check_placed(ctx, streams, full, boxes, extra, form, base, what)


@pytest.mark.parametrize("h,w", [(64, 96), (100, 130)])
def test_placed_boxes_of_golden_mixed_batches(h, w):
    """constants (the pitched fill), frames without a residual layer, legacy forms and residuals in one batch"""
    names, streams = B.golden_batch(h, w)
    with L.Context(len(streams), h, w) as ctx:
        full = B.golden_full(ctx, names, streams)
        all_forms(ctx, streams, full, mixed_boxes(h, w, range(len(streams))), "golden")
        assert same_bits(ctx.decode_frames(streams), full)


@pytest.mark.parametrize("h,w,n", [(40, 32, 4), (97, 131, 4), (160, 520, 3)], ids=["level-1-unfused", "odd", "strips-and-pieces"])
def test_placed_boxes_of_coded_frames(h, w, n):
    streams, ref = B.coded(h, w, n, L.MAX_ERROR, 0.5)
    with L.Context(n, h, w) as ctx:
        full = B.product_full(ctx, streams, ref)
        boxes = mixed_boxes(h, w, range(n))
        if w > 500:                                                        # one, two and three strips of the top level in one launch
            boxes += [(f, r0, c0, 70, cols) for f in range(n) for r0, c0, cols in ((0, 10, 100), (60, 100, 130), (90, 284, 236), (33, 241, 101))]
        all_forms(ctx, streams, full, boxes, (h, w))
    with L.Context(2, h, w) as ctx:                                        # batches of the shard and host forms own parts of the list, not of the output
        for form in FORMS[1:]:
            check_placed(ctx, streams, full, mixed_boxes(h, w, [0, 2, n - 1]), 1, form, 3, "batches")


def test_uniform_list_equals_the_box_list():
    h, w = 100, 130
    streams = B.five_of_100x130()
    boxes = B.random_boxes(h, w, 5, 21, 33, 30, 4)
    with L.Context(5, h, w) as ctx:
        want = B.boxes_of(ctx, streams, boxes, 21, 33)
        table = [(f, r0, c0, 21, 33, e * 21 * 33, 33) for e, (f, r0, c0) in enumerate(boxes)]
        for form in FORMS:
            rc, got = raw_placed(ctx, streams, table, 30 * 21 * 33, form)
            assert rc == 0 and np.array_equal(got, want.view(np.uint32).ravel()), form


# ---- rounds ---------------------------------------------------------------------------------------------------------------------
def rounds_case():
    """3 frames of 100 x 130, 23 boxes of mixed sizes: through 4 slots (six rounds, a frame's boxes split across them) and
    through 16; same bits from both"""
    h, w = 100, 130
    streams = B.five_of_100x130()[:3]
    rng = np.random.default_rng(23)
    boxes = []
    for k in range(23):
        rows, cols = int(rng.integers(1, 60)), int(rng.integers(1, 90))
        boxes.append((k * 3 // 23, int(rng.integers(0, h - rows + 1)), int(rng.integers(0, w - cols + 1)), rows, cols))
    got = []
    for cap in (4, 16):
        with L.Context(cap, h, w) as ctx:
            full = ctx.decode_frames(streams)
            got.append(check_placed(ctx, streams, full, boxes, 1, FORMS[0], 1, f"capacity {cap}"))
            check_placed(ctx, streams, full, boxes, 0, FORMS[2], 2, f"capacity {cap}, host")
    assert np.array_equal(got[0], got[1])


def test_rounds():
    rounds_case()


def _poisoned_child():
    rounds_case()
    print("SLAB_CHILD ok", flush=True)


@pytest.mark.parametrize("pattern", ["0xFF", "0x7F"])
def test_rounds_on_a_poisoned_workspace(pattern):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EBCC_")}
    env["EBCC_HIP_POISON_ALLOC"] = pattern
    code = f"import sys; sys.path.insert(0, {L.ROOT!r}); from tests import test_slab_decode_gpu as S; S._poisoned_child()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=L.ROOT, timeout=600)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-1500:]}{r.stderr[-3000:]}"
    assert "SLAB_CHILD ok" in r.stdout


# ---- refusals, named and unnamed frames ----------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    streams = B.five_of_100x130()
    big = (1 << 64) - 1
    ok = [(0, 0, 0, 10, 10, 0, 10), (1, 5, 5, 7, 9, 100, 12), (4, 90, 120, 10, 10, 200, 10)]
    cases = [("no boxes", [], 300), ("rows zero", ok + [(4, 0, 0, 0, 5, 0, 5)], 300), ("cols zero", ok + [(4, 0, 0, 5, 0, 0, 5)], 300),
             ("below the frame", ok + [(4, 91, 0, 10, 10, 0, 10)], 300), ("right of the frame", ok + [(4, 0, 121, 10, 10, 0, 10)], 300),
             ("taller than the frame", [(0, 0, 0, 101, 1, 0, 1)], 300), ("wider than the frame", [(0, 0, 0, 1, 131, 0, 131)], 300),
             ("origin that wraps", [(0, big, 0, 2, 1, 0, 1)], 300), ("size that wraps", [(0, 2, 0, big - 1, 1, 0, 1)], 300),
             ("pitch below cols", ok + [(4, 0, 0, 5, 6, 0, 5)], 300),
             ("last sample at out_floats", [(0, 0, 0, 10, 10, 201, 10)], 300), ("last row beyond", [(0, 0, 0, 10, 10, 0, 33)], 300),
             ("offset beyond", [(0, 0, 0, 1, 1, 300, 1)], 300), ("offset that wraps", [(0, 0, 0, 2, 2, big, 2)], 300), ("pitch that wraps", [(0, 0, 0, 3, 2, 0, big)], 300),
             ("frame == n_frames", ok + [(5, 0, 0, 1, 1, 0, 1)], 300), ("frame far outside", ok + [(big, 0, 0, 1, 1, 0, 1)], 300),
             ("frames out of order", [ok[1], ok[0]], 300), ("frames out of order", ok + [(3, 0, 0, 1, 1, 0, 1)], 300)]
    with L.Context(5, 100, 130) as ctx:
        full = ctx.decode_frames(streams)
        for form in FORMS:
            for what, table, floats in cases:
                rc, _ = raw_placed(ctx, streams, table, floats, form)
                assert rc == 1, (form, what)
                assert error(), (form, what)
            rc, got = raw_placed(ctx, streams, [(0, 0, 0, 10, 10, 200, 10)], 300, form)                 # the last sample is the output's last float
            assert rc == 0 and np.array_equal(got, expected(full, [(0, 0, 0, 10, 10, 200, 10)], 300)), form
    with L.Context(3, 100, 130) as ctx:                                   # more frames than the context holds: the one-batch form refuses
        assert raw_placed(ctx, streams, ok, 300, FORMS[0])[0] == 1
        assert raw_placed(ctx, streams, ok, 300, FORMS[1])[0] == 0


def test_unnamed_frames_are_not_read_and_a_truncated_named_one_is_refused():
    streams = B.five_of_100x130()
    boxes = [(1, 10, 20, 30, 41), (1, 50, 60, 5, 5), (3, 0, 0, 100, 130), (3, 70, 100, 30, 30), (3, 70, 100, 1, 2)]
    s = streams[3]
    tail = struct.unpack("<Q", s[40:48])[0]
    assert tail > 200
    bad = list(streams)
    bad[3] = s[:40] + struct.pack("<Q", tail - 40) + s[48:len(s) - 40]                # a consistent header over a codestream that ends early
    with L.Context(5, 100, 130) as ctx:
        full = ctx.decode_frames(streams)
        keep, ptrs, sizes = B._args(bad)
        out = L.DeviceArray(nbytes=5 * 100 * 130 * 4)
        assert L.product().ebcc_hip_decode_frames(ctx.ptr, ptrs, sizes, 5, out.ptr) != 0
        out.free()
        table, floats = laid_out(boxes, 3)
        for form in FORMS:
            absent = [x if f in (1, 3) else None for f, x in enumerate(streams)]
            rc, got = raw_placed(ctx, absent, table, floats, form)
            assert rc == 0 and np.array_equal(got, expected(full, table, floats)), (form, error())
            assert raw_placed(ctx, bad, table, floats, form)[0] != 0, form                              # (raw_placed: nothing written)
            rc, got = raw_placed(ctx, bad, table[:2], floats, form)                                     # (the bad frame is not named)
            assert rc == 0 and np.array_equal(got, expected(full, table[:2], floats)), form


# ---- containers -----------------------------------------------------------------------------------------------------------------
def field(dims, seed=40):
    return np.stack([L.era5_like(dims[1], dims[2], seed + t, 1.2 + 0.1 * t, 1.0 + 0.5 * (t % 3)) for t in range(dims[0])]).astype(np.float32)


def container_of(data, cd, mode, err, fn="ebcc_encode_chunking", base_cr=10.0):
    cfg = L.make_config(data.shape, cd, base_cr=base_cr, error=err, residual_type=mode)
    buf = C.api_encode(data.copy(), cfg, fn)
    return buf, C.api_decode(buf, "ebcc_decode_chunking").reshape(data.shape)


def raw_slab(form, ctx, buf, slab):
    """-> the slab (nt, rows, cols) or None when the call refuses (then nothing was written); form: device, host or cached"""
    t0, r0, c0, nt, nr, nc = slab
    s = Slab(*slab)
    b = ctypes.create_string_buffer(bytes(buf), len(buf))
    n = nt * nr * nc if 0 < nt * nr * nc < (1 << 28) else 0
    if form == "cached":
        res = ctypes.c_void_p()
        m = lib().ebcc_decode_chunking_slab(b, len(buf), ctypes.byref(s), ctypes.byref(res))
        if m == 0:
            assert not res.value
            return None
        assert m == n
        out = np.frombuffer(ctypes.string_at(res.value, 4 * m), np.float32).reshape(nt, nr, nc).copy()
        L.product().free_buffer(res)
        return out
    words = np.full(FRONT + 1 + n + BACK, SENT, np.uint32)
    if form == "host":
        rc = lib().ebcc_hip_decode_container_slab_host(ctx.ptr, b, len(buf), ctypes.byref(s), words.ctypes.data + 4 * (FRONT + 1))
        back = words
    else:
        d = L.DeviceArray(words)
        rc = lib().ebcc_hip_decode_container_slab(ctx.ptr, b, len(buf), ctypes.byref(s), d.ptr + 4 * (FRONT + 1))
        back = d.get(np.uint32, words.shape)
        d.free()
    assert (back[:FRONT + 1] == SENT).all() and (back[FRONT + 1 + n:] == SENT).all(), ("written outside the output", form, slab)
    if rc:
        assert (back == SENT).all(), ("written by a call that failed", form, slab)
        return None
    return back[FRONT + 1:FRONT + 1 + n].view(np.float32).reshape(nt, nr, nc).copy()


def check_slabs(ctx, buf, full, slabs, forms=("device", "host", "cached")):
    for slab in slabs:
        t0, r0, c0, nt, nr, nc = slab
        want = full[t0:t0 + nt, r0:r0 + nr, c0:c0 + nc]
        for form in forms:
            got = raw_slab(form, ctx, buf, slab)
            assert got is not None, (form, slab, error())
            assert same_bits(got, want), (form, slab, int((got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum()))


def random_slabs(dims, k, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        ext = [int(rng.integers(1, d + 1)) for d in dims]
        out.append(tuple([int(rng.integers(0, d - e + 1)) for d, e in zip(dims, ext)] + ext))
    return out


@pytest.mark.parametrize("mode,err", [(L.MAX_ERROR, 0.5), (L.RELATIVE_ERROR, 1e-3), (L.NONE, 0.0)], ids=["abs", "rel", "none"])
def test_container_slabs(mode, err):
    dims, cd = (3, 70, 90), (1, 32, 40)
    buf, full = container_of(field(dims), cd, mode, err)
    slabs = [(0, 0, 0, 3, 70, 90)] + [(t, r, c, 1, 1, 1) for t in (0, 2) for r in (0, 69) for c in (0, 89)]
    slabs += [(1, 35, 45, 1, 20, 30), (0, 60, 75, 3, 10, 15), (1, 0, 0, 1, 70, 90), (0, 30, 38, 2, 5, 5)]     # inside a chunk; a 2 x 2 corner of padded chunks; t0 = 1, nt = 1
    slabs += random_slabs(dims, 20, 5)
    with L.Context(27, 32, 40) as ctx:
        check_slabs(ctx, buf, full, slabs)


def entries(buf):
    """[(offset of the payload, bytes)] of a container's chunks"""
    out, p = [], 80
    while p < len(buf):
        n = struct.unpack("<Q", buf[p:p + 8])[0]
        out.append((p + 8, n))
        p += 8 + n
    return out


def test_unmet_chunks_are_not_read():
    dims, cd = (3, 70, 90), (1, 32, 40)
    buf, full = container_of(field(dims), cd, L.MAX_ERROR, 0.5)
    slab = (1, 30, 38, 1, 20, 10)                                          # meets the chunks (1, 0..1, 0..1): linear 9, 10, 12, 13
    met = {9, 10, 12, 13}
    scrubbed = bytearray(buf)
    ents = entries(buf)
    assert len(ents) == 27
    for k, (at, n) in enumerate(ents):
        if k not in met:
            scrubbed[at:at + n] = b"\xA5" * n
    streams = [buf[at:at + n] for at, n in ents]
    cut = list(streams)
    cut[12] = cut[12][:len(cut[12]) // 2]
    with L.Context(4, 32, 40) as ctx:
        check_slabs(ctx, bytes(scrubbed), full, [slab])
        for form in ("device", "host", "cached"):
            assert raw_slab(form, ctx, sharding.assemble_ebck(dims, cd, cut), slab) is None, form
            assert raw_slab(form, ctx, sharding.assemble_ebck(dims, cd, cut), (0, 0, 0, 1, 70, 90)) is not None, form    # (the cut chunk is not met)


def test_batches_and_constant_chunks():
    """30 chunks through a context of 4: batches on both engine sets; one chunk-aligned block is constant (the pitched fill)"""
    dims, cd = (5, 100, 130), (1, 64, 64)
    data = field(dims, 70)
    data[2, 0:64, 64:128] = np.float32(3.25)
    buf, full = container_of(data, cd, L.MAX_ERROR, 0.5)
    assert (full[2, 0:64, 64:128] == np.float32(3.25)).all()
    slabs = [(0, 0, 0, 5, 100, 130), (2, 10, 60, 1, 70, 50), (1, 50, 50, 3, 30, 31), (2, 0, 64, 1, 64, 64), (4, 99, 129, 1, 1, 1)]
    with L.Context(4, 64, 64) as ctx:
        check_slabs(ctx, buf, full, slabs)


@pytest.mark.parametrize("dims,cd,slabs", [((1, 2100, 1100), (1, 1024, 1100), [(0, 924, 800, 1, 200, 300), (0, 1900, 900, 1, 200, 200)]),
                                            ((1, 2100, 2100), (1, 1024, 1024), [(0, 924, 874, 1, 200, 300), (0, 1900, 1900, 1, 200, 200)])],
                         ids=["2100x1100", "2100x2100"])
def test_default_chunk_geometry(dims, cd, slabs):
    """ebcc_encode_chunking_compat's own chunks: 1024 along an axis longer than 2047, the whole axis otherwise - 2100 x 1100 gives
    chunks of 1024 x 1100 (the slab across (1024, 1024) crosses the row boundary alone), 2100 x 2100 chunks of 1024 x 1024 and a
    four-chunk corner at (1024, 1024); each with a slab that reaches the last row and column"""
    buf, full = container_of(field(dims, 90), None, L.MAX_ERROR, 0.5, "ebcc_encode_chunking_compat", 30.0)
    assert struct.unpack("<3Q", buf[40:64]) == cd
    with L.Context(4, cd[1], cd[2]) as ctx:
        check_slabs(ctx, buf, full, slabs)


def test_refused_containers():
    plain = B.five_of_100x130()[0]
    dims, cd = (3, 70, 90), (1, 32, 40)
    buf, _ = container_of(field(dims), cd, L.NONE, 0.0)
    several = sharding.assemble_ebck((2, 32, 32), (2, 32, 32), [plain])
    ok = (0, 0, 0, 1, 10, 10)
    with L.Context(4, 32, 40) as ctx, L.Context(2, 32, 32) as small:
        for form in ("device", "host", "cached"):
            for what, c, data, slab in [("chunks of several frames", small, several, ok), ("a plain frame stream", ctx, plain, ok),
                                        ("a context of another geometry", small, buf, ok), ("an empty slab", ctx, buf, (0, 0, 0, 1, 0, 10)),
                                        ("a slab outside", ctx, buf, (2, 0, 0, 2, 10, 10)), ("trailing bytes", ctx, buf + b"\0", ok),
                                        ("a truncated chain", ctx, buf[:-1], ok)]:
                if form == "cached" and what == "a context of another geometry":
                    continue
                assert raw_slab(form, c, data, slab) is None, (form, what)
                assert error(), (form, what)
            assert raw_slab(form, ctx, buf, ok) is not None, form


# ---- Python ---------------------------------------------------------------------------------------------------------------------
def test_python_read_slab_and_decode_placed():
    from ebcc_amd import container, h5_batch
    dims, cd = (3, 70, 90), (1, 32, 40)
    buf, full = container_of(field(dims), cd, L.MAX_ERROR, 0.5)
    assert container.info(buf) == (dims, cd)
    assert same_bits(container.decode_chunking(buf), full)
    cuts = [(None, None, None), (slice(1, 2), slice(30, 50), slice(38, 48)), (slice(0, 3), slice(69, 70), None), (slice(-1, None), slice(None, 33), slice(5, -5))]
    with h5_batch.BatchCodec(32, 40, max_frames=4) as codec:
        for t, r, c in cuts:
            want = full[t if t else slice(None), r if r else slice(None), c if c else slice(None)]
            assert same_bits(container.read_slab(buf, t, r, c), want), (t, r, c)
            assert same_bits(container.read_slab(buf, t, r, c, codec=codec), want), (t, r, c)
            into = np.full(want.shape, -1.0, np.float32)
            assert same_bits(container.read_slab(buf, t, r, c, out=into, codec=codec), want) and same_bits(into, want)
        for bad in [dict(t=slice(0, 3, 2)), dict(rows=slice(5, 5)), dict(cols=slice(80, 70)), dict(t=1), dict(out=np.zeros(5, np.float32))]:
            with pytest.raises(ValueError):
                container.read_slab(buf, **bad)
        with pytest.raises(ValueError):
            container.info(buf[:70])
        with pytest.raises(ValueError):
            container.read_slab(B.five_of_100x130()[0])
    with h5_batch.BatchCodec(64, 64, max_frames=2) as other:
        with pytest.raises(ValueError):
            container.read_slab(buf, codec=other)
    h, w = 100, 130
    streams = B.five_of_100x130()
    table, floats = laid_out([(0, 3, 5, 17, 23), (0, 0, 0, 100, 130), (2, 50, 60, 1, 1), (4, 10, 0, 40, 130), (4, 99, 129, 1, 1)], 3)
    with h5_batch.BatchCodec(h, w, max_frames=2) as codec:
        full = codec.decode(streams)
        out = np.full(floats + 7, SENT, np.uint32).view(np.float32)
        assert codec.decode_placed(streams, table, out) is out
        assert np.array_equal(out.view(np.uint32), np.concatenate([expected(full, table, floats), np.full(7, SENT, np.uint32)]))
        named = set(table[:, 0].tolist())
        again = np.full(floats + 7, SENT, np.uint32).view(np.float32)
        codec.decode_placed([s if f in named else None for f, s in enumerate(streams)], table, again)
        assert np.array_equal(again.view(np.uint32), out.view(np.uint32))
        def changed(col, value, row=0):
            t = table.copy()
            t[row, col] = value
            return t
        for bad in [table[::-1], changed(3, 0), changed(4, 131), changed(1, 90), changed(0, 5, 4), changed(2, -1), changed(6, 22), changed(5, floats + 7, 4),
                    np.zeros((0, 7), np.int64), np.zeros((2, 3), np.int64)]:
            with pytest.raises(ValueError):
                codec.decode_placed(streams, bad, out)
        with pytest.raises(ValueError):
            codec.decode_placed(streams, table, np.zeros(floats, np.float64))
        cut = list(streams)
        cut[4] = cut[4][:len(cut[4]) // 2]
        with pytest.raises(RuntimeError):
            codec.decode_placed(cut, table, again)
        assert np.array_equal(again.view(np.uint32), out.view(np.uint32))
