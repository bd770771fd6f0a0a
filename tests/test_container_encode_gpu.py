"""GPU: container encode from the device (ebcc_hip_gather_chunks, ebcc_hip_array_range, ebcc_hip_encode_array_chunks,
ebcc_hip_encode_container, include/ebcc_hip.h; ebcc_amd/container.py: encode_resident).  Every comparison is bitwise.  The
yardstick is the oracle, which is pinned to the reference build: a container made from an array on the device is the oracle's
ebcc_encode_chunking / ebcc_encode_chunking_compat of the same array, byte for byte, and so is what the product's own host entry
points give.  The gather alone is held against clamped indexing in numpy, the range against numpy's min and max.

The input A (3, 70, 100) in chunks of (1, 32, 48) has 27 chunks, 6 real rows in the last chunk row and 4 real columns in the last
chunk column; one chunk is constant, one nearly flat.  On the oracle (asserted below, on its own output) MAX_ERROR 0.02 gives
constant, base-only and residual chunks, and RELATIVE_ERROR 0.002 gives another container in the compat form (global range,
14 880 bytes) than in the plain form (per-chunk range, 28 062 bytes): a pass can come neither from the per-chunk range nor from
a container of base layers alone.  The reference's compat container exceeds its own bound here (largest error 0.79 against
0.57), so parity is asserted, not the bound."""
import ctypes
import struct

import numpy as np
import pytest

from tests import _lib as L
from tests import test_codec_gpu as C

pytestmark = pytest.mark.gpu

SENT = np.uint32(0xA5A5A5A5)
FRONT, BACK = 64, 37                                  # floats of sentinel before (256 bytes) and behind
DIMS, CD = (3, 70, 100), (1, 32, 48)
MODES = {"abs": (L.MAX_ERROR, 0.02), "rel": (L.RELATIVE_ERROR, 0.002), "none": (L.NONE, 0.0)}
FORMS = ("ebcc_encode_chunking", "ebcc_encode_chunking_compat")


class Slab(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in ("t0", "row0", "col0", "nt", "rows", "cols")]


@pytest.fixture(autouse=True)
def _search_settings(monkeypatch):
    monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", "0.02")
    monkeypatch.setenv("EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "1")
    L.oracle().orc_set_j2k_backend(0)


def lib():
    """the product with the new entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    cfg_p = ctypes.POINTER(L.CodecConfig)
    for name, args in (("ebcc_hip_gather_chunks", [ctypes.c_void_p, ctypes.c_void_p, L.c_size_p, L.c_size_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
                       ("ebcc_hip_array_range", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
                       ("ebcc_hip_encode_array_chunks", [ctypes.c_void_p, ctypes.c_void_p, cfg_p, ctypes.c_size_t, ctypes.c_size_t, L.c_void_pp, L.c_size_p]),
                       ("ebcc_hip_encode_container", [ctypes.c_void_p, ctypes.c_void_p, cfg_p, ctypes.c_int, L.c_void_pp, L.c_size_p]),
                       ("ebcc_hip_decode_container_slab", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p])):
        fn = getattr(p, name)
        fn.argtypes, fn.restype = args, ctypes.c_int
    return p


def error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


def three(v):
    return (ctypes.c_size_t * 3)(*v)


# ---- inputs and the oracle's containers, made once ------------------------------------------------------------------------------
_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def array_a():
    def make():
        a = np.stack([L.era5_like(70, 100, 7 + i, 1.0 + 0.1 * (i % 4), 0.6) for i in range(3)])
        a = (a + 0.05 * np.arange(100)[None, None, :] + 0.03 * np.arange(70)[None, :, None]).astype(np.float32)
        a[0, :32, :48] = 7.0
        a[0, :32, 48:96] = 250 + (a[0, :32, 48:96] - 250) * np.float32(1e-4)
        a.setflags(write=False)
        return a
    return once("A", make)


def config(dims, cd, mode, base_cr=15.0):
    return L.make_config(dims, cd, base_cr=base_cr, error=MODES[mode][1], residual_type=MODES[mode][0])


def oracle_a(mode, compat):
    return once(("oracle", mode, compat), lambda: L.orc_encode(array_a(), config(DIMS, CD, mode), "orc_" + FORMS[compat]))


def entries(buf):
    """the chunk streams of a container"""
    out, p = [], 80
    while p < len(buf):
        n = struct.unpack("<Q", buf[p:p + 8])[0]
        out.append(buf[p + 8:p + 8 + n])
        p += 8 + n
    return out


def kinds(buf):
    """c: constant chunk, b: base layer alone, r: with a residual layer"""
    heads = [struct.unpack("<4sBBHIIQIIQQ", s[:48]) for s in entries(buf)]
    return "".join("c" if h[2] & 1 else "b" if h[9] == 0 else "r" for h in heads)


def test_the_oracle_containers_are_the_cases_this_file_needs():
    assert kinds(oracle_a("abs", 0)) == "cbrbbrrrrbrrbbrrrrrrrrrrrrr"
    assert kinds(oracle_a("rel", 0)) == "c" + "r" * 26
    assert kinds(oracle_a("rel", 1)) == "cbrrrrrrrrrrrrrrrbrrrrrrrrr"
    assert oracle_a("rel", 0) != oracle_a("rel", 1) and len(oracle_a("rel", 1)) < len(oracle_a("rel", 0))
    assert oracle_a("abs", 0) == oracle_a("abs", 1) and oracle_a("none", 0) == oracle_a("none", 1)


class Resident:
    """a host array on the device, beginning `base` floats behind a 256-byte boundary, sentinels around it"""

    def __init__(self, host, base=1):
        host = np.ascontiguousarray(host, np.float32)
        self.words = np.concatenate([np.full(FRONT + base, SENT, np.uint32), host.view(np.uint32).ravel(), np.full(BACK, SENT, np.uint32)])
        self.d = L.DeviceArray(self.words)
        assert self.d.ptr % 256 == 0
        self.ptr = self.d.ptr + 4 * (FRONT + base)

    def unchanged(self):
        return np.array_equal(self.d.get(np.uint32, self.words.shape), self.words)

    def free(self):
        self.d.free()


# ---- 1. the gather alone --------------------------------------------------------------------------------------------------------
def clamped_chunks(x, cd, first, count):
    nt, H, W = x.shape
    _, ch, cw = cd
    n1, n2 = -(-H // ch), -(-W // cw)
    out = np.empty((count, ch, cw), np.float32)
    for k in range(count):
        t, cy, cx = np.unravel_index(first + k, (nt, n1, n2))
        out[k] = x[t][np.minimum(cy * ch + np.arange(ch), H - 1)][:, np.minimum(cx * cw + np.arange(cw), W - 1)]
    return out


def gather(ctx, src, dims, cd, first, count, out_base):
    """-> (return value, the count x ch x cw words); asserts that nothing before or behind them was written"""
    n = count * cd[1] * cd[2]
    words = np.full(FRONT + out_base + n + BACK, SENT, np.uint32)
    d = L.DeviceArray(words)
    rc = lib().ebcc_hip_gather_chunks(ctx.ptr, src.ptr, three(dims), three(cd), first, count, d.ptr + 4 * (FRONT + out_base))
    back = d.get(np.uint32, words.shape)
    d.free()
    assert (back[:FRONT + out_base] == SENT).all() and (back[FRONT + out_base + n:] == SENT).all(), "written outside the output"
    if rc:
        assert (back == SENT).all(), "written by a call that failed"
    return rc, back[FRONT + out_base:FRONT + out_base + n]


GATHER = {"a-edges-on-both-axes": (DIMS, CD, 5, 7), "b-one-real-column": ((2, 33, 97), (1, 33, 48), 1, 4),
          "c-chunk-larger-than-the-array": ((2, 40, 50), (1, 64, 64), 1, 1), "d-no-padding": ((2, 64, 96), (1, 32, 48), 2, 5)}


@pytest.mark.parametrize("case", sorted(GATHER))
def test_gather_is_clamped_indexing(case):
    dims, cd, first, count = GATHER[case]
    x = array_a() if dims == DIMS else (np.arange(dims[0] * dims[1] * dims[2], dtype=np.float32) * np.float32(0.5) - 1000).reshape(dims)
    total = dims[0] * -(-dims[1] // cd[1]) * -(-dims[2] // cd[2])
    with L.Context(2, 32, 48) as ctx:
        for base in (0, 1, 2, 3):
            src = Resident(x, base)
            for lo, cnt in ((0, total), (first, count)):
                for out_base in sorted({0, (base + 1) % 4}):
                    rc, got = gather(ctx, src, dims, cd, lo, cnt, out_base)
                    assert rc == 0, (case, base, error())
                    want = clamped_chunks(x, cd, lo, cnt).view(np.uint32).ravel()
                    assert np.array_equal(got, want), (case, base, out_base, lo, cnt, int((got != want).sum()))
            assert src.unchanged()
            src.free()


# ---- 2. the range ---------------------------------------------------------------------------------------------------------------
def array_range(ctx, ptr, n):
    mm = np.array([-123.0, -456.0], np.float32)
    rc = lib().ebcc_hip_array_range(ctx.ptr, ptr, n, mm.ctypes.data)
    if rc:
        assert mm.tolist() == [-123.0, -456.0], "minmax written by a call that failed"
    return rc, mm


def test_array_range():
    """One array is a group of one of the range kernel: 2047 / 2048 / 2049 floats lie around the one block of 256 lanes x 8 floats,
    4097 is the first grid of two blocks.  The flag of a planted NaN / Inf comes from whichever wave meets it."""
    flat = array_a().ravel()
    with L.Context(2, 32, 48) as ctx:
        for base in (0, 1, 2, 3):
            src = Resident(flat, base)
            for n in (1, 2, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 4097, flat.size):
                rc, mm = array_range(ctx, src.ptr, n)
                assert rc == 0, error()
                assert mm[0] == flat[:n].min() and mm[1] == flat[:n].max(), (base, n)
            assert src.unchanged()
            src.free()
        for n in (1, 65, 4097, flat.size):                                 # the last float is the 4-byte tail or in a 16-byte load
            for at in sorted({0, n // 2, n - 1}):
                for bad in (np.nan, np.inf, -np.inf):
                    x = flat[:n].copy()
                    x[at] = bad
                    src = Resident(x, 1)
                    assert array_range(ctx, src.ptr, n)[0] == 2 and error(), (n, at, bad)
                    if n > 1 and at == n - 1:
                        rc, mm = array_range(ctx, src.ptr, n - 1)         # (and nothing behind the n floats is read)
                        assert rc == 0 and mm[0] == x[:-1].min() and mm[1] == x[:-1].max()
                    src.free()
        assert lib().ebcc_hip_array_range(ctx.ptr, None, 5, np.zeros(2, np.float32).ctypes.data) == 1
        d = L.DeviceArray(flat[:8])
        assert lib().ebcc_hip_array_range(ctx.ptr, d.ptr, 0, np.zeros(2, np.float32).ctypes.data) == 1
        d.free()


# ---- 3. container parity --------------------------------------------------------------------------------------------------------
def encode_container(ctx, ptr, cfg, compat):
    """-> (return value, the container or None); after a failure *out is NULL and the size 0"""
    out, n = ctypes.c_void_p(0xDEAD), ctypes.c_size_t(77)
    rc = lib().ebcc_hip_encode_container(ctx.ptr, ptr, ctypes.byref(cfg), compat, ctypes.byref(out), ctypes.byref(n))
    if rc:
        assert not out.value and n.value == 0, "*out after a failure"
        return rc, None
    buf = ctypes.string_at(out.value, n.value)
    L.product().free_buffer(out)
    return 0, buf


def encode_array_chunks(ctx, ptr, cfg, first, count):
    """-> (return value, the streams or None); after a failure every out_streams entry is NULL"""
    room = max(1, min(count, 64))
    outs, sizes = (ctypes.c_void_p * room)(), (ctypes.c_size_t * room)()
    rc = lib().ebcc_hip_encode_array_chunks(ctx.ptr, ptr, ctypes.byref(cfg), first, count, outs, sizes)
    if rc:
        assert all(not outs[k] for k in range(room)), "streams left behind by a call that failed"
        return rc, None
    res = [ctypes.string_at(outs[k], sizes[k]) for k in range(count)]
    for k in range(count):
        L.product().free_buffer(outs[k])
    return 0, res


def decode_whole(ctx, buf, dims):
    s = Slab(0, 0, 0, *dims)
    b = ctypes.create_string_buffer(bytes(buf), len(buf))
    out = L.DeviceArray(nbytes=4 * dims[0] * dims[1] * dims[2])
    rc = lib().ebcc_hip_decode_container_slab(ctx.ptr, b, len(buf), ctypes.byref(s), out.ptr)
    assert rc == 0, error()
    got = out.get(np.float32, dims)
    out.free()
    return got


@pytest.mark.parametrize("compat", [0, 1], ids=["plain", "compat"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_container_of_a_device_array_is_the_oracles(mode, compat):
    a, want = array_a(), oracle_a(mode, compat)
    assert C.api_encode(a.copy(), config(DIMS, CD, mode), FORMS[compat]) == want          # the product's own host entry point
    src = Resident(a, 1)                                                                   # 4 bytes behind a 256-byte boundary
    for cap in (4, 32):                                                                    # 7 batches on two engine sets, the last of 3 chunks; one batch
        with L.Context(cap, CD[1], CD[2]) as ctx:
            cfg = config(DIMS, CD, mode)
            rc, got = encode_container(ctx, src.ptr, cfg, compat)
            assert rc == 0, (cap, error())
            assert got == want, (cap, kinds(got), kinds(want))
            assert cfg.residual_compression_type == MODES[mode][0] and cfg.error == np.float32(MODES[mode][1])      # the caller's config is not touched
            if cap == 4:
                rc, part = encode_array_chunks(ctx, src.ptr, cfg, 5, 7)
                assert rc == 0, error()
                if not (compat and mode == "rel"):                                         # (the chunk form has no global range)
                    assert part == entries(want)[5:12]
            else:
                dec = decode_whole(ctx, got, DIMS)
                ref = L.orc_decode(want, "orc_ebcc_decode_chunking").reshape(DIMS)
                assert np.array_equal(dec.view(np.uint32), ref.view(np.uint32))
    assert src.unchanged()
    src.free()


# ---- 4. chunks that are whole frames ----------------------------------------------------------------------------------------------
def test_whole_frame_chunks_are_coded_where_they_lie():
    dims, cd = (5, 33, 40), (1, 33, 40)
    x = np.stack([L.era5_like(33, 40, 50 + i, 1.2, 1.0) for i in range(5)]).astype(np.float32)
    cfg = config(dims, cd, "abs")
    want = L.orc_encode(x, cfg, "orc_ebcc_encode_chunking")
    assert "r" in kinds(want)
    src = Resident(x, 3)
    for cap in (2, 8):
        with L.Context(cap, 33, 40) as ctx:
            rc, got = encode_container(ctx, src.ptr, cfg, 0)
            assert rc == 0 and got == want, (cap, error())
            rc, part = encode_array_chunks(ctx, src.ptr, cfg, 1, 3)
            assert rc == 0 and part == entries(want)[1:4], (cap, error())
            assert part == ctx.encode_shard(x[1:4], config((1, 33, 40), None, "abs"))
    assert src.unchanged()
    src.free()


# ---- 5. a constant array ----------------------------------------------------------------------------------------------------------
def test_constant_array_with_a_range_of_zero():
    dims = (2, 40, 50)
    x = np.full(dims, 3.5, np.float32)
    cfg = config(dims, None, "rel")                                        # compat's own chunks: (1, 40, 50)
    want = L.orc_encode(x, cfg, "orc_ebcc_encode_chunking_compat")
    assert kinds(want) == "cc"
    src = Resident(x, 2)
    with L.Context(2, 40, 50) as ctx:
        rc, got = encode_container(ctx, src.ptr, cfg, 1)
        assert rc == 0 and got == want, error()
        rc, mm = array_range(ctx, src.ptr, x.size)
        assert rc == 0 and mm.tolist() == [3.5, 3.5]
    src.free()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_nan():
    a = array_a()
    big = (1 << 64) - 1
    src = Resident(a, 1)
    ok = config(DIMS, CD, "abs")
    refused = [("a context of another geometry", "other", ok, 0, 27, None),
               ("chunks of several frames", "ctx", config((4, 64, 48), (2, 32, 48), "abs"), 0, 2, "one-frame"),
               ("zero frames", "ctx", config((0, 70, 100), CD, "abs"), 0, 1, None),
               ("zero columns", "ctx", config((3, 70, 0), CD, "abs"), 0, 1, None),
               ("chunk rows below 32", "small", config(DIMS, (1, 16, 48), "abs"), 0, 1, None),
               ("chunk columns above 2047", "ctx", config((3, 70, 5000), (1, 32, 2048), "abs"), 0, 1, None),
               ("dims whose product overflows", "ctx", config((1 << 62, 70, 100), CD, "abs"), 0, 1, "overflow"),
               ("first + count beyond the chunks", "ctx", ok, 20, 8, None), ("first beyond the chunks", "ctx", ok, 28, 1, None),
               ("first + count that wraps", "ctx", ok, big, 2, None), ("no chunks", "ctx", ok, 3, 0, None)]
    with L.Context(4, CD[1], CD[2]) as ctx, L.Context(2, 32, 40) as other, L.Context(2, 32, 64) as small:
        who = {"ctx": ctx, "other": other, "small": small}
        for what, c, cfg, first, count, word in refused:
            rc, _ = encode_array_chunks(who[c], src.ptr, cfg, first, count)
            assert rc == 1 and error(), what
            assert word is None or word in error(), (what, error())
            if (first, count) in ((0, 27), (0, 2), (0, 1)):                # (the container form has no range of chunks)
                for compat in (0, 1):
                    rc, _ = encode_container(who[c], src.ptr, cfg, compat)
                    assert rc == 1 and error(), what
                    assert word is None or word in error(), (what, error())
            if c == "ctx" and cfg.chunk_dims[1] >= 32:                     # the gather has the same checks (any context serves it)
                rc, _ = gather(ctx, src, tuple(cfg.dims), tuple(cfg.chunk_dims), first, min(count, 64), 1)
                assert rc == 1 and error(), what
        rc, _ = encode_array_chunks(ctx, src.ptr, config(DIMS, None, "abs"), 0, 1)       # the chunk form has no default chunks
        assert rc == 1 and error()
        assert encode_container(ctx, None, ok, 0)[0] == 1 and encode_array_chunks(ctx, None, ok, 0, 1)[0] == 1
        # NaN in one interior sample: 2 from both container forms, by the chunk's own check and by the range
        x = a.copy()
        x[1, 40, 50] = np.nan
        bad = Resident(x, 1)
        assert encode_container(ctx, bad.ptr, ok, 0)[0] == 2
        assert encode_container(ctx, bad.ptr, config(DIMS, CD, "rel"), 1)[0] == 2 and error()
        assert encode_array_chunks(ctx, bad.ptr, ok, 0, 27)[0] == 2
        bad.free()
        # and the context is as good as before
        for mode, compat in (("abs", 0), ("rel", 1)):
            rc, got = encode_container(ctx, src.ptr, config(DIMS, CD, mode), compat)
            assert rc == 0 and got == oracle_a(mode, compat), error()
    assert src.unchanged()
    src.free()


# ---- 7. Python ------------------------------------------------------------------------------------------------------------------
def test_python_encode_resident_and_read_slab():
    from ebcc_amd import container, h5_batch
    a = array_a()

    def h5_config(mode, cd=CD):
        c = h5_batch.CodecConfig()
        c.dims[:] = (0, 0, 0)                                              # (taken from the dims argument)
        c.chunk_dims[:] = cd
        c.base_cr, c.residual_compression_type, c.residual_cr, c.error = 15.0, MODES[mode][0], 0.0, MODES[mode][1]
        return c

    class Tensor:                                                          # what a torch tensor offers
        def __init__(self, ptr):
            self.ptr = ptr

        def data_ptr(self):
            return self.ptr

    src = Resident(a, 1)
    with h5_batch.BatchCodec(CD[1], CD[2], max_frames=4) as codec:
        whole = h5_config("abs")
        whole.dims[:] = DIMS
        assert container.plan(whole) == (CD, 27) == container.plan(whole, compat=True)
        with pytest.raises(ValueError):
            container.plan(h5_config("abs", (1, 16, 48)))
        buf = container.encode_resident(src.ptr, DIMS, h5_config("abs"), codec)
        assert buf == oracle_a("abs", 0)
        assert container.encode_resident(Tensor(src.ptr), DIMS, h5_config("rel"), codec, compat=True) == oracle_a("rel", 1)
        full = container.decode_chunking(buf)
        box = container.read_slab(buf, slice(0, 3), slice(20, 45), slice(40, 60), codec=codec)                 # across the chunk corner at (32, 48)
        assert np.array_equal(box.view(np.uint32), np.ascontiguousarray(full[:, 20:45, 40:60]).view(np.uint32))
        with pytest.raises(ValueError):
            container.encode_resident(src.ptr, (3, 70, 100), h5_config("abs", (1, 32, 40)), codec)             # not the codec's geometry
        x = a.copy()
        x[2, 69, 99] = np.inf
        bad = Resident(x, 1)
        with pytest.raises(ValueError):
            container.encode_resident(bad.ptr, DIMS, h5_config("rel"), codec, compat=True)
        bad.free()
    src.free()
