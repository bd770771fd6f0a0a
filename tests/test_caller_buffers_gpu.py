"""GPU: what the library may touch of a caller's buffers.  Every entry point that reads or writes frames runs on buffers
that sit at every alignment the kernels branch on, between guard bands, and the whole allocation is read back afterwards.

Placement: one allocation [front guard | payload | back guard], guards of at least 4096 bytes, the payload `off` bytes
after a 256-byte boundary for off in {0, 4, 8, 16}: 4 fails every alignment test of the kernels (k_in_minmax's 16-byte
loads, the 8-byte pair forms of J2kSinkFrameTop and of the residual layer's last row pass, decode_batch's direct output),
8 passes the pair test only, 16 fails the 256-byte test only, 0 is what every other test runs.
- Outputs: guards and payload are 0xA5 bytes before the call; afterwards every byte outside [n][H][W] must still be 0xA5.
  The output allocation holds the context's capacity of frames, so the frames behind a partial batch are guard as well.
- Inputs: the guards are 0xFF bytes (NaN): a read past either end that reaches a result shows as return code 2, as a
  changed min/max or as a changed stream.  After the call the whole allocation must be unchanged.
- Host pointers: the same in a flat numpy array, the payload one float off the array's alignment, -777.25 around outputs
  and NaN around inputs.

Every value is compared exactly with the CPU oracle (streams byte for byte, fields as uint32), at 100 x 130 and 721 x 1440
with golden hashes as well (codec_streams.json; caller_buffers.json, oracle/make_golden_caller_buffers.py) - never with
the product's own result at another alignment.  The one figure that is not a bit pattern, the error sum of
ebcc_hip_j2k_emulated_decode (a float64 sum whose order is the kernel's), keeps the bound of tests/test_j2k_gpu.py.

Shapes: 33 x 47 (odd W, odd n_pix: every second frame of a batch is 4-byte misaligned by itself), 33 x 46 (even W,
n_pix % 4 == 2), 64 x 96 (n_pix % 4 == 0, one code-block row), 100 x 130 (several code-blocks), and one batch of
721 x 1440 at off = 4 (the only size at which the fused levels run more than one strip and piece).

Limit: a read past the end whose value is later dropped changes no result and is invisible here.  Only reads that reach a
result, and all writes, are pinned."""
import ctypes
import functools
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from tests import _domains as D
from tests import _lib as L
from tests import test_j2k_gpu as J

pytestmark = pytest.mark.gpu

GUARD = 4096                                   # bytes of guard on either side (device), a multiple of 256
HOST_GUARD = 1024                              # floats of guard on either side (host)
OFFSETS = (0, 4, 8, 16)
OTHER_OFF = {0: 4, 4: 8, 8: 16, 16: 0}         # the offset of the second buffer where a call takes two
SHAPES = [(33, 47), (33, 46), (64, 96), (100, 130)]
BIG = (721, 1440)
OUT_BYTE, IN_BYTE = 0xA5, 0xFF
HOST_OUT = np.float32(-777.25)
CAP = 8                                        # frames a frame-codec context holds
UNIT_CAP, UNIT_N = 5, 3                        # unit-level entry points: three frames on a context of five
MODES = (L.MAX_ERROR, L.RELATIVE_ERROR, L.NONE)
MODE_IDS = {L.MAX_ERROR: "abs", L.RELATIVE_ERROR: "rel", L.NONE: "none"}
QUANTILE = "0.1"                               # EBCC_INIT_BASE_ERROR_QUANTILE: a loose base layer, so that residual layers stay
# (base_cr, error) per mode: the golden cases of 100 x 130; at 64 x 96 no frame keeps its residual layer under them
CONFIG = {L.MAX_ERROR: (5.0, 0.01), L.RELATIVE_ERROR: (30.0, 1e-3), L.NONE: (10.0, 0.0)}
CONFIG_AT = {((64, 96), L.MAX_ERROR): (5.0, 0.002), ((64, 96), L.RELATIVE_ERROR): (5.0, 1e-4)}
GOLDEN_100x130 = {L.MAX_ERROR: "cr5_m1_e0.01", L.RELATIVE_ERROR: "cr30_m2_e0.001", L.NONE: "cr10_m0_e0.0"}
STREAMS = json.load(open(os.path.join(L.GOLDEN, "codec_streams.json")))
BIG_FIXTURE = os.path.join(L.GOLDEN, "caller_buffers.json")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(autouse=True)
def _search_env(monkeypatch):
    for k in ("EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK_CONSISTENCY",
              "EBCC_DISABLE_MEAN_ADJUSTMENT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", QUANTILE)
    L.oracle().orc_set_j2k_backend(0)


# ---- placement ---------------------------------------------------------------------------------------------------------------
class Placed:
    """One device allocation [front guard | payload | back guard]: `ptr` is the payload, `off` bytes after a 256-byte
    boundary.  data: the payload's bytes (an input, guards of 0xFF); None: an output of `nbytes`, everything 0xA5."""

    def __init__(self, off, data=None, nbytes=None):
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).ravel()
            nbytes = data.size
        self.fill = IN_BYTE if data is not None else OUT_BYTE
        self.lo, self.nbytes = GUARD + off, nbytes
        self.image = np.full(self.lo + nbytes + GUARD + (-nbytes) % 4, self.fill, np.uint8)
        if data is not None:
            self.image[self.lo:self.lo + nbytes] = data
        self.dev = L.DeviceArray(self.image)
        assert self.dev.ptr % 256 == 0, "the allocator's own alignment"
        self.ptr = self.dev.ptr + self.lo
        assert self.ptr % 256 == off

    def back(self):
        return self.dev.get(np.uint8, (self.image.size,))

    def unchanged(self):
        """an input after the call: not a byte of the allocation differs"""
        return np.array_equal(self.back(), self.image)

    def written(self, nbytes):
        """an output after the call: the first `nbytes` of the payload; every byte before and behind must be the sentinel"""
        b = self.back()
        assert (b[:self.lo] == self.fill).all(), "written in front of the output"
        behind = b[self.lo + nbytes:]
        assert (behind == self.fill).all(), ("written behind the output", int(np.flatnonzero(behind != self.fill)[0]))
        return b[self.lo:self.lo + nbytes].copy()

    def frames(self, n, h, w):
        return self.written(n * h * w * 4).view(np.float32).reshape(n, h, w)

    def free(self):
        self.dev.free()


class HostPlaced:
    """The same layout in a flat float32 array, the payload one float off the array's own alignment."""

    def __init__(self, data=None, count=None):
        self.fill = np.float32(np.nan) if data is not None else HOST_OUT
        self.count = data.size if data is not None else count
        self.lo = HOST_GUARD + 1
        self.array = np.full(self.lo + self.count + HOST_GUARD, self.fill, np.float32)
        if data is not None:
            self.array[self.lo:self.lo + self.count] = np.ascontiguousarray(data, np.float32).ravel()
        self.image = self.array.copy()
        self.ptr = self.array.ctypes.data + 4 * self.lo
        assert self.ptr % 8 == 4

    def unchanged(self):
        return np.array_equal(bits(self.array), bits(self.image))

    def written(self, count):
        assert same_bits(self.array[:self.lo], self.image[:self.lo]), "written in front of the output"
        assert same_bits(self.array[self.lo + count:], self.image[self.lo + count:]), "written behind the output"
        return self.array[self.lo:self.lo + count].copy()


# ---- calls on raw pointers ---------------------------------------------------------------------------------------------------
def lib():
    p = L.product()
    p.ebcc_hip_encode_host_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(L.CodecConfig),
                                              L.c_void_pp, L.c_size_p]
    p.ebcc_hip_decode_host_frames.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p]
    for name in ("ebcc_hip_upload", "ebcc_hip_download"):
        getattr(p, name).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return p


def _take_streams(outs, sizes, n):
    res = []
    for f in range(n):
        res.append(ctypes.string_at(outs[f], sizes[f]))
        L.product().free_buffer(outs[f])
    return res


def _stream_args(streams):
    n = len(streams)
    bufs = [ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p).value for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    return bufs, ptrs, sizes


def encode_at(ctx, entry, ptr, n, cfg):
    """a frame-codec encode entry point on frames at `ptr` (device or host) -> the streams"""
    outs, sizes = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)()
    rc = getattr(lib(), entry)(ctx.ptr, ptr, n, ctypes.byref(cfg), outs, sizes)
    assert rc == 0, (entry, rc, L.product().ebcc_hip_last_error())
    return _take_streams(outs, sizes, n)


def decode_at(ctx, entry, streams, ptr):
    """a frame-codec decode entry point into `ptr` (device or host) -> the return code"""
    keep, ptrs, sizes = _stream_args(streams)
    return getattr(lib(), entry)(ctx.ptr, ptrs, sizes, len(streams), ptr)


# ---- the reference: frames, the oracle's streams and fields, once per (shape, mode) ------------------------------------------
def batch_frames(h, w):
    """Eight frames: [0] keeps its residual layer in MAX_ERROR and RELATIVE_ERROR, [1] is constant, [2] does not keep it
    (reference() asserts all three); then five more value domains.  At 100 x 130 [0] and [2] are the golden inputs."""
    e = L.era5_like(h, w, 11)
    flat = (np.float32(250.0) + (e - np.float32(250.0)) * np.float32(1e-4)).astype(np.float32)
    if (h, w) == (100, 130):
        inputs = np.load(os.path.join(L.GOLDEN, "codec_inputs.npz"))
        first, third = inputs["in2"], inputs["in3"]
    else:
        first, third = D.noise(h, w, 1), L.era5_like(h, w, 12, 1.0, 0.7)
    return np.stack([first, np.full((h, w), 273.15, np.float32), third, e, flat, D.wind(h, w, 1), D.humidity(h, w, 1),
                     D.precipitation(h, w, 1)]).astype(np.float32)


def big_frames():
    h, w = BIG
    e = L.era5_like(h, w, 11)
    flat = (np.float32(250.0) + (e - np.float32(250.0)) * np.float32(1e-4)).astype(np.float32)
    return np.stack([L.era5_like(h, w, 12, 1.0, 0.7), np.full((h, w), 273.15, np.float32), flat]).astype(np.float32)


def config_of(shape, mode):
    cr, err = CONFIG_AT.get((tuple(shape), mode), CONFIG[mode])
    return L.make_config((1,) + tuple(shape), base_cr=cr, error=err, residual_type=mode)


def kind_of(stream):
    return "const" if stream[5] & 1 else "residual" if int.from_bytes(stream[16:24], "little") else "base"


@functools.lru_cache(maxsize=None)
def reference(shape, mode):
    """-> (frames [8][h][w], config, the oracle's streams, the oracle's decoded fields [8][h][w])"""
    h, w = shape
    frames = batch_frames(h, w)
    cfg = config_of(shape, mode)
    streams = [L.orc_encode(x, cfg) for x in frames]
    fields = np.stack([np.asarray(L.orc_decode(s)).reshape(h, w) for s in streams])
    kinds = [kind_of(s) for s in streams]
    assert kinds[:3] == (["residual", "const", "base"] if mode != L.NONE else ["base", "const", "base"]), kinds
    if shape == (100, 130):
        for k, name in ((0, "in2"), (2, "in3")):
            c = STREAMS[f"{name}_{GOLDEN_100x130[mode]}_q{QUANTILE}"]
            assert sha(streams[k]) == sha(bytes.fromhex(c["stream_hex"])) and sha(fields[k].tobytes()) == c["decoded_sha256"], c
    frames.setflags(write=False)
    fields.setflags(write=False)
    return frames, cfg, streams, fields


def rotation(k):
    """k frame indices that run through all eight and differ from batch to batch"""
    return [(3 * i) % CAP for i in range(k)]


# ---- 1. frame codec, device-resident -----------------------------------------------------------------------------------------
def check_frame_codec(ctx, cap, frames, cfg, streams, fields, off, batches, shard):
    n_all, h, w = frames.shape
    for n in batches:
        src = Placed(off, data=frames[:n])
        assert encode_at(ctx, "ebcc_hip_encode_frames", src.ptr, n, cfg) == streams[:n], ("encode_frames", n)
        assert src.unchanged(), ("encode_frames changed its input", n)
        src.free()
        dst = Placed(off, nbytes=cap * h * w * 4)                  # (capacity frames: those behind frame n are guard)
        assert decode_at(ctx, "ebcc_hip_decode_frames", streams[:n], dst.ptr) == 0, L.product().ebcc_hip_last_error()
        assert same_bits(dst.frames(n, h, w), fields[:n]), ("decode_frames", n)
        dst.free()
    if shard:
        pick = rotation(shard)
        src = Placed(off, data=frames[pick])
        assert encode_at(ctx, "ebcc_hip_encode_shard", src.ptr, shard, cfg) == [streams[i] for i in pick], "encode_shard"
        assert src.unchanged(), "encode_shard changed its input"
        src.free()
        dst = Placed(off, nbytes=-(-shard // cap) * cap * h * w * 4)
        assert decode_at(ctx, "ebcc_hip_decode_shard", [streams[i] for i in pick], dst.ptr) == 0, L.product().ebcc_hip_last_error()
        assert same_bits(dst.frames(shard, h, w), fields[pick]), "decode_shard"
        dst.free()


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("mode", MODES, ids=[MODE_IDS[m] for m in MODES])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_codec_on_placed_device_buffers(shape, mode, off):
    """ebcc_hip_encode_frames / decode_frames with 3 and 8 frames on a context of 8, ebcc_hip_encode_shard / decode_shard with
    19 frames (three batches, both engine sets)"""
    frames, cfg, streams, fields = reference(shape, mode)
    with L.Context(CAP, *shape) as ctx:
        check_frame_codec(ctx, CAP, frames, cfg, streams, fields, off, (3, CAP), 19)


@pytest.mark.parametrize("mode", MODES, ids=[MODE_IDS[m] for m in MODES])
def test_frame_codec_at_full_size(mode):
    """three frames of 721 x 1440 on a context of four, 4 bytes off: streams and fields of the reference build (hashes)"""
    fixture = json.load(open(BIG_FIXTURE))
    want = fixture["cases"][MODE_IDS[mode]]
    frames = big_frames()
    for x, c in zip(frames, want):
        assert sha(x.tobytes()) == c["field_sha256"], "input differs"
    assert [c["kind"] for c in want] == (["residual", "const", "base"] if mode != L.NONE else ["base", "const", "base"])
    cfg = L.make_config((1,) + BIG, base_cr=fixture["config"][MODE_IDS[mode]][0], error=fixture["config"][MODE_IDS[mode]][1],
                        residual_type=mode)
    h, w = BIG
    with L.Context(4, h, w) as ctx:
        src = Placed(4, data=frames)
        got = encode_at(ctx, "ebcc_hip_encode_frames", src.ptr, 3, cfg)
        assert src.unchanged()
        src.free()
        assert [(len(s), sha(s)) for s in got] == [(c["n"], c["stream_sha256"]) for c in want]
        dst = Placed(4, nbytes=4 * h * w * 4)
        assert decode_at(ctx, "ebcc_hip_decode_frames", got, dst.ptr) == 0, L.product().ebcc_hip_last_error()
        dec = dst.frames(3, h, w)
        dst.free()
        assert [sha(d.tobytes()) for d in dec] == [c["decoded_sha256"] for c in want]


# ---- 2. unit-level entry points ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def residual_reference(shape):
    h, w = shape
    r = np.random.default_rng(h * 10007 + w)
    imgs = np.stack([L.kat_image(h, w), r.random((h, w), dtype=np.float32), L.smooth_image(h, w, 3)])
    truncs = (0, 8 * (h * w // 10))
    enc = {tb: [L.orc_spiht_encode(x, tb) for x in imgs] for tb in truncs}
    coeffs = [L.orc_spiht_coeffs(x) for x in imgs]
    imgs.setflags(write=False)
    return imgs, truncs, enc, coeffs


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_residual_layer_entry_points_on_placed_buffers(shape, off):
    """ebcc_hip_spiht_encode / _coeffs read a placed input, ebcc_hip_spiht_decode / _decode_prefix write a placed output: the
    oracle calls of tests/test_residual_gpu.py, at two truncations each"""
    h, w = shape
    imgs, truncs, enc, coeffs = residual_reference(shape)
    n = UNIT_N
    p = L.product()
    with L.Context(UNIT_CAP, h, w) as ctx:
        src = Placed(off, data=imgs)
        npad = p.ebcc_hip_padded_pixels(ctx.ptr)
        c, dc = np.zeros((n, npad), np.int32), np.zeros(n, np.int32)
        assert p.ebcc_hip_spiht_coeffs(ctx.ptr, src.ptr, n, c.ctypes.data, dc.ctypes.data) == 0, p.ebcc_hip_last_error()
        for f, (ref, rdc) in enumerate(coeffs):
            assert dc[f] == rdc and np.array_equal(c[f].reshape(ref.shape), ref), ("coeffs", f)
        for tb in truncs:
            outs, sizes = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)()
            assert p.ebcc_hip_spiht_encode(ctx.ptr, src.ptr, n, (ctypes.c_size_t * n)(*[tb] * n), outs, sizes) == 0, p.ebcc_hip_last_error()
            assert _take_streams(outs, sizes, n) == enc[tb], ("spiht_encode", tb)
            # (the encoder's bookkeeping of this call:) the decode of a prefix, whole and a third
            for frac in (1.0, 0.33):
                nbytes = [max(17, int(len(s) * frac)) for s in enc[tb]]
                dst = Placed(OTHER_OFF[off], nbytes=UNIT_CAP * h * w * 4)
                assert p.ebcc_hip_spiht_decode_prefix(ctx.ptr, n, (ctypes.c_size_t * n)(*[8 * b for b in nbytes]), dst.ptr) == 0, p.ebcc_hip_last_error()
                got = dst.frames(n, h, w)
                dst.free()
                for f, s in enumerate(enc[tb]):
                    assert same_bits(got[f], L.orc_spiht_decode(s[:nbytes[f]], h, w, 8 * nbytes[f])), ("decode_prefix", tb, frac, f)
        assert src.unchanged()
        src.free()
        full = enc[truncs[1]]
        for streams in (full, [s[:max(17, len(s) // 3)] for s in full]):
            keep, ptrs, sizes = _stream_args(streams)
            dst = Placed(off, nbytes=UNIT_CAP * h * w * 4)
            nb = (ctypes.c_size_t * n)(*[8 * len(s) for s in streams])
            assert p.ebcc_hip_spiht_decode(ctx.ptr, ptrs, sizes, nb, n, dst.ptr) == 0, p.ebcc_hip_last_error()
            got = dst.frames(n, h, w)
            dst.free()
            for f, s in enumerate(streams):
                assert same_bits(got[f], L.orc_spiht_decode(s, h, w)), ("spiht_decode", len(s), f)


J2K_RATES = (3.0, 40.0)
J2K_TARGET = (0.05, 0.3, 1.0)


@functools.lru_cache(maxsize=None)
def j2k_reference(shape):
    h, w = shape
    fields = J._fields(h, w)
    scaled = [L.scale_u16(x) for x in fields]
    enc = {cr: [L.orc_j2k_encode(u16, cr) for u16, _, _ in scaled] for cr in J2K_RATES}
    dec = {cr: np.stack([L.map_decoded(L.orc_j2k_decode(s), mn, mx) for s, (_, mn, mx) in zip(enc[cr], scaled)]) for cr in J2K_RATES}
    fields.setflags(write=False)
    return fields, [(mn, mx) for _, mn, mx in scaled], enc, dec


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_base_layer_entry_points_on_placed_buffers(shape, off):
    """ebcc_hip_j2k_encode reads a placed input, ebcc_hip_j2k_emulated_decode reads it and writes a placed output at another
    offset, ebcc_hip_j2k_decode writes a placed output: the oracle calls of tests/test_j2k_gpu.py, at two rates"""
    h, w = shape
    fields, minmax, enc, dec = j2k_reference(shape)
    n = UNIT_N
    p = L.product()
    with L.Context(UNIT_CAP, h, w) as ctx:
        src = Placed(off, data=fields)
        for cr in J2K_RATES:
            outs, sizes = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)()
            crs, mm = np.full(n, cr, np.float32), np.zeros(2 * n, np.float32)
            assert p.ebcc_hip_j2k_encode(ctx.ptr, src.ptr, n, crs.ctypes.data, outs, sizes, mm.ctypes.data) == 0, p.ebcc_hip_last_error()
            assert _take_streams(outs, sizes, n) == enc[cr], ("j2k_encode", cr)
            assert same_bits(mm.reshape(n, 2), np.asarray(minmax, np.float32)), ("min / max", cr)
            dst = Placed(OTHER_OFF[off], nbytes=UNIT_CAP * h * w * 4)
            tg, nbad, esum = np.asarray(J2K_TARGET, np.float32), np.zeros(n, np.uint64), np.zeros(n, np.float64)
            assert p.ebcc_hip_j2k_emulated_decode(ctx.ptr, src.ptr, n, tg.ctypes.data, dst.ptr, nbad.ctypes.data, esum.ctypes.data) == 0, \
                p.ebcc_hip_last_error()
            assert same_bits(dst.frames(n, h, w), dec[cr]), ("emulated decode", cr)
            dst.free()
            for f in range(n):
                err = fields[f] - dec[cr][f]
                assert int(nbad[f]) == int((np.abs(err) > tg[f]).sum()), ("nbad", cr, f)
                assert abs(esum[f] - err.astype(np.float64).sum()) <= 1e-6 * max(1.0, abs(esum[f])), ("err_sum", cr, f)
        assert src.unchanged()
        src.free()
        for cr in J2K_RATES:
            keep, ptrs, sizes = _stream_args(enc[cr])
            mm = np.asarray(minmax, np.float32)
            dst = Placed(off, nbytes=UNIT_CAP * h * w * 4)
            assert p.ebcc_hip_j2k_decode(ctx.ptr, ptrs, sizes, n, mm.ctypes.data, dst.ptr) == 0, p.ebcc_hip_last_error()
            assert same_bits(dst.frames(n, h, w), dec[cr]), ("j2k_decode", cr)
            dst.free()


# ---- 3. host-pointer forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=[MODE_IDS[m] for m in MODES])
def test_host_frame_entry_points_on_placed_host_arrays(mode):
    """ebcc_hip_encode_host_frames / decode_host_frames: 27 frames of 64 x 96 on a context of 8 (four batches, both engine
    sets), then 3 (a partial batch into an array that holds 8)"""
    shape = (64, 96)
    frames, cfg, streams, fields = reference(shape, mode)
    with L.Context(CAP, *shape) as ctx:
        for m, room in ((27, 27), (3, CAP)):
            pick = rotation(m)
            src = HostPlaced(data=frames[pick])
            assert encode_at(ctx, "ebcc_hip_encode_host_frames", src.ptr, m, cfg) == [streams[i] for i in pick], m
            assert src.unchanged(), m
            dst = HostPlaced(count=room * frames[0].size)
            assert decode_at(ctx, "ebcc_hip_decode_host_frames", [streams[i] for i in pick], dst.ptr) == 0, L.product().ebcc_hip_last_error()
            assert same_bits(dst.written(m * frames[0].size).reshape(m, *shape), fields[pick]), m


CHUNK = (4, 96, 160)


@functools.lru_cache(maxsize=None)
def chunk_reference():
    data = np.stack([L.era5_like(96, 160, 300 + s, 1.0 + 0.1 * (s % 4), 0.6) for s in range(CHUNK[0])]).astype(np.float32)
    out = []
    for mode in MODES:
        cr, err = CONFIG[mode]
        cfg = L.make_config(CHUNK, base_cr=cr, error=err, residual_type=mode)
        s = L.orc_encode(data, cfg)
        out.append((cfg, s, np.asarray(L.orc_decode(s))))
    return data, out


def test_reference_api_on_a_placed_host_array():
    """ebcc_encode of a chunk of four frames (one multi-tile image) read from a placed host array, and ebcc_decode of it, into
    its own allocation and into a placed array of the caller's (*out_buffer set)"""
    from tests.test_codec_gpu import api_decode
    data, cases = chunk_reference()
    p = L.product()
    for cfg, want, field in cases:
        src = HostPlaced(data=data)
        out = ctypes.c_void_p()
        n = p.ebcc_encode(src.ptr, ctypes.byref(cfg), ctypes.byref(out))
        assert n > 0 and out
        got = ctypes.string_at(out.value, n)
        p.free_buffer(out)
        assert got == want and src.unchanged(), cfg.residual_compression_type
        assert same_bits(api_decode(got), field), cfg.residual_compression_type
        dst = HostPlaced(count=data.size)
        b = ctypes.create_string_buffer(got, len(got))
        out = ctypes.c_void_p(dst.ptr)
        assert p.ebcc_decode(b, len(got), ctypes.byref(out)) == data.size and out.value == dst.ptr
        assert same_bits(dst.written(data.size), field), cfg.residual_compression_type


@pytest.mark.parametrize("off", OFFSETS)
def test_upload_and_download_on_a_placed_device_buffer(off):
    """ebcc_hip_upload / ebcc_hip_download of a byte count that is no multiple of 16 (nor of 4)"""
    nbytes = 3 * 100 * 130 * 4 + 7
    data = np.random.default_rng(5).integers(0, 256, nbytes, dtype=np.uint8)
    p = lib()
    with L.Context(3, 100, 130) as ctx:
        dev = Placed(off, nbytes=nbytes)
        assert p.ebcc_hip_upload(ctx.ptr, dev.ptr, data.ctypes.data, nbytes) == 0, p.ebcc_hip_last_error()
        assert np.array_equal(dev.written(nbytes), data)
        host = np.full(64 + nbytes + 64, 0x5A, np.uint8)
        assert p.ebcc_hip_download(ctx.ptr, host.ctypes.data + 64, dev.ptr, nbytes) == 0, p.ebcc_hip_last_error()
        assert np.array_equal(host[64:64 + nbytes], data) and (host[:64] == 0x5A).all() and (host[64 + nbytes:] == 0x5A).all()
        assert np.array_equal(dev.written(nbytes), data)                 # (the download's source is as it was)
        dev.free()


# ---- 4. a refused batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_refused_batch_writes_nothing_outside_the_output(shape, off):
    """the MAX_ERROR batch with one codestream cut short under a consistent header: refused, both guards intact, and the
    intact batch then decodes on the same context"""
    h, w = shape
    frames, cfg, streams, fields = reference(shape, L.MAX_ERROR)
    bad = list(streams)
    s = bad[2]
    tail, cut = struct.unpack("<Q", s[40:48])[0], 40
    assert tail > 200
    bad[2] = s[:40] + struct.pack("<Q", tail - cut) + s[48:len(s) - cut]
    with L.Context(CAP, h, w) as ctx:
        dst = Placed(off, nbytes=CAP * h * w * 4)
        assert decode_at(ctx, "ebcc_hip_decode_frames", bad, dst.ptr) != 0
        dst.written(CAP * h * w * 4)                                     # (asserts the guards)
        assert decode_at(ctx, "ebcc_hip_decode_frames", streams, dst.ptr) == 0, L.product().ebcc_hip_last_error()
        assert same_bits(dst.frames(CAP, h, w), fields)
        dst.free()
