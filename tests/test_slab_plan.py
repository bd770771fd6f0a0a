"""CPU tests of the slab plan (ebcc_hip_slab_plan, include/ebcc_hip.h): a sub-array of an array stored in one-frame chunks as
placed boxes, one per chunk it meets - and of ebcc_hip_container_info, which checks an EBCK container as ebcc_decode_chunking
does.  The model is the array of its own flat indices: every chunk is built from it by clamped indexing (as the encoder pads
the edge chunks), the boxes are applied to an output of -1 with a write counter, and the output must be idx[slab] with every
element written exactly once.  The library loads without a device; a missing symbol fails."""
import ctypes
import struct

import numpy as np
import pytest

from ebcc_amd import sharding
from tests import _lib as L

GEOMETRIES = [((3, 70, 90), (1, 32, 40)), ((2, 64, 96), (1, 64, 96)), ((5, 100, 130), (1, 64, 64)), ((2, 2100, 1100), (1, 1024, 1024))]
SENTINEL = 0xC3


class Slab(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in ("t0", "row0", "col0", "nt", "rows", "cols")]


def _plan():
    fn = getattr(L.product(), "ebcc_hip_slab_plan")       # AttributeError where the feature is missing: a failure, not a skip
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return fn


def _info():
    fn = getattr(L.product(), "ebcc_hip_container_info")
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return fn


def _three(v):
    return (ctypes.c_size_t * 3)(*v)


def slab_plan(dims, cd, slab, room=None):
    """-> (count, boxes (count, 7) int64 or None); the counting call and the filling call must agree, and a refusal must leave
    the table's bytes as they were"""
    s = Slab(*slab)
    n = _plan()(_three(dims), _three(cd), ctypes.byref(s), None, 0)
    cap = max(n, 0) + 3 if room is None else room
    table = np.full((cap, 7), SENTINEL * 0x0101010101010101, np.uint64)
    m = _plan()(_three(dims), _three(cd), ctypes.byref(s), table.ctypes.data, cap)
    if m < 0:
        assert (table.view(np.uint8) == SENTINEL).all(), "boxes written by a call that refuses"
        return m, None
    assert m == n, (m, n)
    assert (table[m:].view(np.uint8) == SENTINEL).all(), "written past the boxes"
    return m, table[:m].astype(np.int64)


_model = {}


def model(dims, cd):
    """(idx, chunks): the array of its own indices and its chunks [linear chunk index][cd1][cd2] by clamped indexing"""
    key = (dims, cd)
    if key not in _model:
        idx = np.arange(int(np.prod(dims)), dtype=np.int64).reshape(dims)
        cnt = [-(-d // c) for d, c in zip(dims, cd)]
        chunks = []
        for t in range(cnt[0]):
            for cy in range(cnt[1]):
                ys = np.minimum(cy * cd[1] + np.arange(cd[1]), dims[1] - 1)
                for cx in range(cnt[2]):
                    xs = np.minimum(cx * cd[2] + np.arange(cd[2]), dims[2] - 1)
                    chunks.append(idx[t][np.ix_(ys, xs)])
        _model[key] = (idx, chunks, cnt)
    return _model[key]


def check(dims, cd, slab):
    idx, chunks, cnt = model(dims, cd)
    t0, r0, c0, nt, nr, nc = slab
    n, boxes = slab_plan(dims, cd, slab)
    met = nt * ((r0 + nr - 1) // cd[1] - r0 // cd[1] + 1) * ((c0 + nc - 1) // cd[2] - c0 // cd[2] + 1)
    assert n == met, (slab, n, met)
    out = np.full(nt * nr * nc, -1, np.int64)
    hits = np.zeros(nt * nr * nc, np.int32)
    assert (np.diff(boxes[:, 0]) > 0).all(), "frames must be strictly increasing"
    for frame, row0, col0, rows, cols, at, pitch in boxes.tolist():
        cy, cx = (frame // cnt[2]) % cnt[1], frame % cnt[2]
        assert 0 <= frame < len(chunks) and rows >= 1 and cols >= 1 and pitch == nc
        # inside the chunk's real (unpadded) part
        assert row0 + rows <= min(cd[1], dims[1] - cy * cd[1]) and col0 + cols <= min(cd[2], dims[2] - cx * cd[2]), (slab, frame)
        where = at + np.arange(rows)[:, None] * pitch + np.arange(cols)[None, :]
        assert where.max() < out.size
        out[where] = chunks[frame][row0:row0 + rows, col0:col0 + cols]
        hits[where] += 1
    assert (hits == 1).all(), (slab, "every element exactly once")
    assert np.array_equal(out.reshape(nt, nr, nc), idx[t0:t0 + nt, r0:r0 + nr, c0:c0 + nc]), slab


def named_slabs(dims, cd):
    T, H, W = dims
    out = [(0, 0, 0, T, H, W)]
    out += [(t, r, c, 1, 1, 1) for t in (0, T - 1) for r in (0, H - 1) for c in (0, W - 1)]                  # every corner sample
    out += [(0, H // 2, 0, T, 1, W), (0, 0, W // 3, T, H, 1)]                                                 # one row, one column
    out += [(T - 1, 3, 5, 1, min(cd[1], H) - 7, min(cd[2], W) - 9)]                                           # inside one chunk
    if H > cd[1] and W > cd[2]:
        out += [(0, cd[1] - 5, cd[2] - 7, T, 11, 13)]                                                         # across a four-chunk corner
    out += [(0, max(H - 9, 0), max(W - 11, 0), 1, min(9, H), min(11, W))]                                     # ends in the padded chunk's real edge
    return out


@pytest.mark.parametrize("dims,cd", GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_named_slabs(dims, cd):
    for slab in named_slabs(dims, cd):
        check(dims, cd, slab)


@pytest.mark.parametrize("dims,cd", GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_random_slabs(dims, cd):
    rng = np.random.default_rng(dims[1] * 7 + dims[2])
    big = dims[1] * dims[2] > 1 << 20
    for _ in range(200):
        ext = [int(rng.integers(1, d + 1)) for d in dims]
        if big:                                                            # (the model writes every element: keep most slabs moderate)
            ext[1], ext[2] = min(ext[1], int(rng.integers(1, 400))), min(ext[2], int(rng.integers(1, 400)))
        org = [int(rng.integers(0, d - e + 1)) for d, e in zip(dims, ext)]
        check(dims, cd, tuple(org + ext))


def test_refusals_leave_the_boxes_alone():
    dims, cd = (3, 70, 90), (1, 32, 40)
    big = (1 << 64) - 1
    ok = (0, 0, 0, 3, 70, 90)
    assert slab_plan(dims, cd, ok)[0] == 27
    cases = [("nt zero", dims, cd, (0, 0, 0, 0, 70, 90)), ("rows zero", dims, cd, (0, 0, 0, 3, 0, 90)), ("cols zero", dims, cd, (0, 0, 0, 3, 70, 0)),
             ("past the last step", dims, cd, (1, 0, 0, 3, 70, 90)), ("past the last row", dims, cd, (0, 1, 0, 3, 70, 90)),
             ("past the last column", dims, cd, (0, 0, 1, 3, 70, 90)), ("origin outside", dims, cd, (3, 0, 0, 1, 1, 1)),
             ("origin that wraps", dims, cd, (0, big, 0, 1, 2, 1)), ("extent that wraps", dims, cd, (0, 2, 0, 1, big, 1)),
             ("zero dims", (0, 70, 90), cd, (0, 0, 0, 1, 1, 1)), ("zero dims", (3, 0, 90), cd, (0, 0, 0, 1, 1, 1)), ("zero dims", (3, 70, 0), cd, (0, 0, 0, 1, 1, 1)),
             ("chunks of several frames", dims, (2, 32, 40), ok), ("chunk_dims[0] zero", dims, (0, 32, 40), ok),
             ("chunk rows below 32", dims, (1, 31, 40), ok), ("chunk columns below 32", dims, (1, 32, 31), ok),
             ("chunk rows above 2047", dims, (1, 2048, 40), ok), ("chunk columns above 2047", dims, (1, 32, 2048), ok),
             ("zero chunk dims", dims, (1, 0, 40), ok), ("zero chunk dims", dims, (1, 32, 0), ok)]
    for what, d, c, slab in cases:
        assert slab_plan(d, c, slab)[0] == -1, what
        assert L.product().ebcc_hip_last_error(), what
    assert slab_plan(dims, cd, ok, room=26)[0] == -1, "max_boxes too small"
    assert slab_plan(dims, cd, ok, room=27)[0] == 27


# ---- ebcc_hip_container_info ----------------------------------------------------------------------------------------------------
def info(buf):
    dims, cd = _three((7, 7, 7)), _three((7, 7, 7))
    b = ctypes.create_string_buffer(bytes(buf), len(buf))
    rc = _info()(b, len(buf), dims, cd)
    if rc:
        assert tuple(dims) == (7, 7, 7) and tuple(cd) == (7, 7, 7), "written by a call that refuses"
        return rc, None, None
    return rc, tuple(dims), tuple(cd)


def dummy_container(dims, cd):
    n = int(np.prod([-(-d // c) for d, c in zip(dims, cd)]))
    return sharding.assemble_ebck(dims, cd, [bytes((k * 31 + i) & 0xFF for i in range(5 + 3 * k)) for k in range(n)])


@pytest.mark.parametrize("dims,cd", GEOMETRIES + [((4, 64, 64), (2, 32, 64))], ids=lambda v: "x".join(map(str, v)))
def test_container_info(dims, cd):
    assert info(dummy_container(dims, cd)) == (0, dims, cd)


def test_container_info_refuses_what_decode_chunking_refuses():
    dims, cd = (3, 70, 90), (1, 32, 40)
    good = dummy_container(dims, cd)
    assert info(good)[0] == 0
    last = 5 + 3 * 26                                                       # bytes of the last payload
    counts = lambda num, size: good[:64] + struct.pack("<QQ", num, size) + good[80:]
    cases = [("short header", good[:79], "not an EBCK"), ("no magic", b"EBCC" + good[4:], "not an EBCK"), ("empty", b"", "not an EBCK"),
             ("missing size", good[:80 + 3], "missing chunk size"), ("missing size of the last chunk", good[:len(good) - last - 3], "missing chunk size"),
             ("no entries at all", good[:80], "missing chunk size"),
             ("truncated payload", good[:-1], "truncated chunk payload"), ("truncated first payload", good[:80 + 8 + 2], "truncated chunk payload"),
             ("trailing bytes", good + b"\0", "trailing payload bytes"),
             ("inconsistent chunk count", counts(26, 32 * 40), "inconsistent chunk metadata"), ("inconsistent chunk size", counts(27, 32 * 41), "inconsistent chunk metadata"),
             ("version", good[:4] + struct.pack("<I", 2) + good[8:], "version"), ("ndims", good[:8] + struct.pack("<I", 2) + good[12:], "dimensionality"),
             ("bad chunk dims", sharding.assemble_ebck(dims, (1, 16, 40), []), "bad chunk dimensions"),
             ("zero dims", sharding.ebck_header((3, 70, 90), (1, 32, 40))[:16] + struct.pack("<3Q", 0, 70, 90) + good[40:], "non-zero")]
    for what, buf, text in cases:
        rc, _, _ = info(buf)
        assert rc == 1, what
        assert text in L.product().ebcc_hip_last_error().decode(), (what, L.product().ebcc_hip_last_error())
