"""The frame-geometry catalogue of tests/test_geometry_sweep.py and tests/test_geometry_sweep_gpu.py: small frames chosen by
integer arithmetic for what their size makes the wavelet kernels do, not for their content.  Nothing here calls the product.

A  parity and pad diagonal: each axis takes every value 32 .. 64 once, so the low five bits of n - 1 (which of the five 9/7
   levels have an odd extent) take all 32 patterns per axis and the residual layer's pad to a multiple of 16 all 16 values.
B  strips and pieces of the fused inverse level (60 column pairs a strip, four strips a workgroup, up to 8 vertical pieces) and
   of the residual layer's inverse (120 columns of the padded grid a strip, (ny / 2) / 16 pieces).
C  W = 32: the coarsest band is one column wide and level 1 takes the separate row and column passes; and its transpose.
D  chunks of two frames of height 32 .. 63: the second tile's row offset takes every residue mod 32.

The digests of tests/golden/geometry_sweep.json (oracle/make_golden_geometry.py) are made by digests() / chunk_digests() from
a coder: the reference's programs when the fixture is written, the oracle when tests/test_geometry_sweep.py holds it to them."""
import ctypes
import functools
import hashlib
import os

import numpy as np

from tests import _fields as F
from tests import _lib as L

A = [(32 + k, 32 + (7 * k + 3) % 33) for k in range(33)]
B = [(62, 120), (63, 119), (94, 122), (95, 121), (127, 123), (159, 124), (191, 239), (223, 240), (253, 241), (255, 242), (33, 243),
     (40, 481), (36, 482)]
C = [(47, 32), (100, 32), (255, 32), (32, 65), (32, 127), (32, 129)]
D = [(2, 32 + k, 33 + (11 * k + 5) % 64) for k in range(32)]
PLAIN = A + B + C
FAMILIES = {"A": A, "B": B, "C": C, "D": D}

J2K_KINDS = ("noise", "smooth", "checker")
RESIDUAL_KINDS = ("noise", "spike", "checker")         # (the reference coder asserts on a negative mean: no smooth frame)
J2K_RATES = (1.0, 12.0)
CODEC_BASE_CR, CHUNK_BASE_CR = 30.0, 10.0
CODEC_MODES = (("abs", L.MAX_ERROR), ("rel", L.RELATIVE_ERROR))
REL_ERROR = 1e-3
ENV = ("EBCC_INIT_BASE_ERROR_QUANTILE", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK",
       "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK_CONSISTENCY", "EBCC_DISABLE_MEAN_ADJUSTMENT")


def shape_id(s):
    return "x".join(str(v) for v in s)


def family(shape):
    return next(name for name, shapes in FAMILIES.items() if shape in shapes)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def clear_env():
    """for the fixture's generator; the tests clear the switches through monkeypatch"""
    for k in ENV:
        os.environ.pop(k, None)


def _env_is_clear():
    return not any(k in os.environ for k in ENV)


# ---- inputs (shared, never written to)
def _frozen(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def j2k_frames(h, w):
    return _frozen(np.stack([F.field(k, h, w) for k in J2K_KINDS]))


@functools.lru_cache(maxsize=None)
def residual_frames(h, w):
    return _frozen(np.stack([F.field(k, h, w) for k in RESIDUAL_KINDS]))


@functools.lru_cache(maxsize=None)
def codec_frame(h, w):
    return _frozen(L.era5_like(h, w, 131 * h + w))


@functools.lru_cache(maxsize=None)
def chunk_frames(tiles, h, w):
    return _frozen(np.stack([L.era5_like(h, w, 7 * h + s) for s in range(tiles)]))


def one_percent(x):
    """1 % of the range, as the float32 the config holds"""
    return float(np.float32(0.01) * (np.float32(x.max()) - np.float32(x.min())))


def codec_config(shape, x, mode):
    return L.make_config(shape, base_cr=CODEC_BASE_CR, error=one_percent(x) if mode == L.MAX_ERROR else REL_ERROR, residual_type=mode)


def chunk_config(shape, x):
    return L.make_config(shape, base_cr=CHUNK_BASE_CR, error=one_percent(x), residual_type=L.MAX_ERROR)


def spiht_budgets(h, w):
    return (0, 8 * (h * w // 10))


def third(stream):
    """bytes of the first third of a residual stream (at least one past its 16-byte header)"""
    return max(17, len(stream) // 3)


# ---- digests: one sha256 per shape and stage, over the shape's cases one after the other in the order of the loops below
class Coder:
    """the five programs a fixture is made from: j2k_encode(u16, cr) -> bytes, j2k_decode(bytes) -> int32 [h][w],
    spiht_encode(img, trunc_bits) -> bytes, spiht_decode(bytes, h, w, num_bits) -> float32 [h][w], codec_encode(x, cfg) -> bytes"""

    def __init__(self, j2k_encode, j2k_decode, spiht_encode, spiht_decode, codec_encode):
        self.j2k_encode, self.j2k_decode, self.spiht_encode, self.spiht_decode, self.codec_encode = \
            j2k_encode, j2k_decode, spiht_encode, spiht_decode, codec_encode


def oracle_coder():
    L.oracle().orc_set_j2k_backend(0)
    return Coder(L.orc_j2k_encode, L.orc_j2k_decode, L.orc_spiht_encode, L.orc_spiht_decode, L.orc_encode)


@functools.lru_cache(maxsize=None)
def reference_coder():
    """the five programs from OpenJPEG 2.4.0 (the oracle's optional backend), the reference's residual coder and the reference build
    (oracle/_ref); made once"""
    lib = L.oracle()
    assert hasattr(lib, "orc_opj_encode") and L.opj_version().startswith("2.4.0"), "needs the OpenJPEG 2.4.0 backend: " + repr(L.opj_version())
    assert L.reference() is not None and os.path.exists(L.REF_SPIHT_SO), "needs the reference build (oracle/_ref)"
    sp = ctypes.CDLL(L.REF_SPIHT_SO)
    sp.spiht_encode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, L.c_void_pp, L.c_size_p, ctypes.c_size_t,
                                ctypes.c_size_t]
    sp.spiht_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                ctypes.c_size_t]
    sp.log_set_quiet.argtypes = [ctypes.c_bool]
    sp.log_set_quiet(True)
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]

    def j2k_encode(img, cr):
        img = np.ascontiguousarray(img, np.uint16)
        out = ctypes.c_void_p()
        n = lib.orc_opj_encode(img.ctypes.data, img.shape[0], img.shape[1], ctypes.c_float(cr), ctypes.byref(out))
        s = ctypes.string_at(out.value, n)
        lib.orc_free(out)
        return s

    def j2k_decode(s):
        b = ctypes.create_string_buffer(s, len(s))
        out, h, w = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        n = lib.orc_opj_decode(b, len(s), ctypes.byref(out), ctypes.byref(h), ctypes.byref(w))
        assert n, "OpenJPEG decoded nothing"
        a = np.frombuffer(ctypes.string_at(out.value, 4 * n), np.int32).reshape(h.value, w.value).copy()
        lib.orc_free(out)
        return a

    def spiht_encode(img, tb):
        img = np.ascontiguousarray(img, np.float32)
        buf, n = ctypes.c_void_p(), ctypes.c_size_t()
        sp.spiht_encode(img.ctypes.data, img.shape[0], img.shape[1], ctypes.byref(buf), ctypes.byref(n), tb, 3)
        s = ctypes.string_at(buf.value, n.value)
        libc.free(buf)
        return s

    def spiht_decode(s, h, w, num_bits):
        b = ctypes.create_string_buffer(bytes(s), len(s))
        out = np.zeros((h, w), np.float32)
        sp.spiht_decode(b, len(s), out.ctypes.data, h, w, num_bits)
        return out

    return Coder(j2k_encode, j2k_decode, spiht_encode, spiht_decode, L.ref_encode)


def _framed(parts):
    """the parts one after the other, each behind its length (8 bytes, little-endian)"""
    return b"".join(len(p).to_bytes(8, "little") + p for p in parts)


def input_digests(shape):
    if len(shape) == 3:
        return {"input": sha(chunk_frames(*shape).tobytes())}
    return {"input_j2k": sha(j2k_frames(*shape).tobytes()), "input_residual": sha(residual_frames(*shape).tobytes()),
            "input_codec": sha(codec_frame(*shape).tobytes())}


def digests(shape, coder):
    """the stage digests of a plain shape"""
    h, w = shape
    assert _env_is_clear(), "a switch of the reference's environment is set"
    out = input_digests(shape)
    streams, samples = [], []
    for x in j2k_frames(h, w):
        u16 = L.scale_u16(x)[0]
        for cr in J2K_RATES:
            s = coder.j2k_encode(u16, cr)
            d = np.ascontiguousarray(coder.j2k_decode(s), np.int32)
            assert d.size == h * w, (shape, cr)
            streams.append(s)
            samples.append(d.tobytes())
    out["j2k_streams"], out["j2k_decoded"] = sha(_framed(streams)), sha(_framed(samples))
    streams, fields = [], []
    for x in residual_frames(h, w):
        for tb in spiht_budgets(h, w):
            s = coder.spiht_encode(np.ascontiguousarray(x), tb)
            n = third(s)
            streams.append(s)
            fields.append(np.ascontiguousarray(coder.spiht_decode(s[:n], h, w, 8 * n), np.float32).tobytes())
    out["spiht_streams"], out["spiht_decoded"] = sha(_framed(streams)), sha(_framed(fields))
    x = codec_frame(h, w)
    for name, mode in CODEC_MODES:
        s = coder.codec_encode(x, codec_config((1, h, w), x, mode))
        assert s, (shape, name)
        out["codec_" + name] = sha(s)
    return out


def chunk_digests(shape, coder):
    assert _env_is_clear(), "a switch of the reference's environment is set"
    out = input_digests(shape)
    x = chunk_frames(*shape)
    s = coder.codec_encode(x, chunk_config(shape, x))
    assert s, shape
    out["chunk_abs"] = sha(s)
    return out


def all_digests(shape, coder):
    return chunk_digests(shape, coder) if len(shape) == 3 else digests(shape, coder)


# per shape: what digests() and chunk_digests() compare with the reference (pairs of codestream and decoded samples, residual
# streams and truncated decodes, frame streams, chunk streams)
COUNTS = {"j2k": len(J2K_KINDS) * len(J2K_RATES), "spiht": len(RESIDUAL_KINDS) * 2, "codec": len(CODEC_MODES), "chunk": 1}
