"""GPU: window decode (ebcc_hip_decode_*_window, include/ebcc_hip.h).  The criterion is exact: the window of every frame is,
bit for bit (compared as uint32), the crop of what ebcc_hip_decode_frames gives on the same context - and the crop of the
oracle's decode.  Every device-resident call decodes into the middle of a sentinel-filled buffer at an address that is 4
bytes off 8-byte alignment and checks that not a byte outside [n][rows][cols] has changed."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest

from tests import _fields as F
from tests import _lib as L
from tests import test_window_plan as P

pytestmark = pytest.mark.gpu

STREAMS = json.load(open(os.path.join(L.GOLDEN, "codec_streams.json")))
SENTINEL = 0xA5
PAD_FRONT, PAD_BACK = 1, 37                    # floats of sentinel before (odd: the output is not 8-byte aligned) and after the output
CONDA_PY = "/opt/conda/bin/python3.9"


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def lib():
    """the product with the window entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    sig = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t] + [ctypes.c_size_t] * 4 + [ctypes.c_void_p]
    for name in ("ebcc_hip_decode_frames_window", "ebcc_hip_decode_shard_window", "ebcc_hip_decode_host_frames_window"):
        fn = getattr(p, name)
        fn.argtypes, fn.restype = sig, ctypes.c_int
    return p


def _args(streams):
    n = len(streams)
    bufs = [ctypes.create_string_buffer(bytes(s), len(s)) for s in streams]
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p).value for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    return bufs, ptrs, sizes


def raw_window(ctx, streams, win, entry="ebcc_hip_decode_frames_window"):
    """-> (return value, the window [n][rows][cols] or None); asserts that nothing outside the output was written, and after a
    non-zero return nothing at all"""
    r0, c0, rows, cols = win
    n = len(streams)
    keep, ptrs, sizes = _args(streams)
    count = n * rows * cols if 0 < rows * cols < (1 << 40) else 0
    total = PAD_FRONT + count + PAD_BACK
    host = np.full(total * 4, SENTINEL, np.uint8)
    d = L.DeviceArray(host)
    rc = getattr(lib(), entry)(ctx.ptr, ptrs, sizes, n, r0, c0, rows, cols, d.ptr + 4 * PAD_FRONT)
    back = d.get(np.uint8, (total * 4,))
    d.free()
    assert (back[:4 * PAD_FRONT] == SENTINEL).all() and (back[4 * (PAD_FRONT + count):] == SENTINEL).all(), ("written outside the output", win)
    if rc:
        assert (back == SENTINEL).all(), ("written by a call that failed", win)
        return rc, None
    return rc, back[4 * PAD_FRONT:4 * (PAD_FRONT + count)].view(np.float32).reshape(n, rows, cols).copy()


def window(ctx, streams, win, entry="ebcc_hip_decode_frames_window"):
    rc, out = raw_window(ctx, streams, win, entry)
    assert rc == 0, (win, L.product().ebcc_hip_last_error())
    return out


def host_window(ctx, streams, win):
    r0, c0, rows, cols = win
    n = len(streams)
    keep, ptrs, sizes = _args(streams)
    out = np.full(PAD_FRONT + n * rows * cols + PAD_BACK, np.float32(-777.25), np.float32)
    rc = lib().ebcc_hip_decode_host_frames_window(ctx.ptr, ptrs, sizes, n, r0, c0, rows, cols, out.ctypes.data + 4 * PAD_FRONT)
    assert rc == 0, (win, L.product().ebcc_hip_last_error())
    assert (out[:PAD_FRONT] == np.float32(-777.25)).all() and (out[PAD_FRONT + n * rows * cols:] == np.float32(-777.25)).all()
    return out[PAD_FRONT:PAD_FRONT + n * rows * cols].reshape(n, rows, cols).copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def crop(full, win):
    r0, c0, rows, cols = win
    return full[:, r0:r0 + rows, c0:c0 + cols]


def windows_of(h, w, n_random=40):
    """the catalogue of tests/test_window_plan.py (corners, 1 x 1, full rows and columns, edges on and beside multiples of
    64 * 2^k) plus seeded random windows, and the whole frame"""
    rng = np.random.default_rng(31 * h + w)
    return P.catalogue(h, w, rng) + P.random_windows(h, w, rng, n_random) + [(0, 0, h, w)]


def check_windows(ctx, streams, full, oracle_fields, wins):
    for win in wins:
        got = window(ctx, streams, win)
        assert same_bits(got, crop(full, win)), (win, int((got.view(np.uint32) != np.ascontiguousarray(crop(full, win)).view(np.uint32)).sum()))
        if oracle_fields is not None:
            assert np.array_equal(got, crop(oracle_fields, win)), ("oracle", win)


def oracle_fields(streams, h, w):
    return np.stack([np.asarray(L.orc_decode(s)).reshape(h, w) for s in streams])


# ---- 5. crop equality --------------------------------------------------------------------------------------------------------
def golden_by_shape():
    g = defaultdict(list)
    for name, c in sorted(STREAMS.items()):
        g[(c["h"], c["w"])].append(name)
    return sorted(g.items())


@pytest.mark.parametrize("shape,names", golden_by_shape(), ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else None)
def test_golden_streams_and_their_legacy_forms(shape, names):
    """every single-frame stream of codec_streams.json (three modes, the constant field, the kept-residual cases) and its
    header-less form, as one mixed batch per shape"""
    h, w = shape
    streams = [bytes.fromhex(STREAMS[n]["stream_hex"]) for n in names]
    streams += [L.legacy_repack(s) for s in streams]
    with L.Context(len(streams), h, w) as ctx:
        full = ctx.decode_frames(streams)
        for k, n in enumerate(names):
            assert sha(full[k].tobytes()) == STREAMS[n]["decoded_sha256"] == sha(full[len(names) + k].tobytes()), n
        ref = oracle_fields(streams[:len(names)], h, w)                  # (the oracle reads the headed form)
        check_windows(ctx, streams, full, np.concatenate([ref, ref]), windows_of(h, w))


ERA5_MODES = [(L.MAX_ERROR, 0.5), (L.RELATIVE_ERROR, 1e-3)]
ERA5_FRAMES = 24
_era5 = {}


def era5_batch(mode, err):
    """24 era5_like 721 x 1440 frames coded by the product at base_cr 30: (streams, sha256 of the full decode)"""
    if mode not in _era5:
        frames = np.stack([L.era5_like(721, 1440, s, 1.2 + 0.1 * (s % 5), 1.0 + 0.5 * (s % 4)) for s in range(ERA5_FRAMES)])
        cfg = L.make_config((1, 721, 1440), base_cr=30.0, error=err, residual_type=mode)
        with L.Context(ERA5_FRAMES, 721, 1440) as ctx:
            streams = ctx.encode_frames(frames, cfg)
            full = ctx.decode_frames(streams)
        _era5[mode] = (streams, full)
    return _era5[mode]


@pytest.mark.parametrize("mode,err", ERA5_MODES, ids=["abs", "rel"])
def test_era5_like_batch(mode, err):
    streams, full0 = era5_batch(mode, err)
    with L.Context(ERA5_FRAMES, 721, 1440) as ctx:
        full = ctx.decode_frames(streams)
        assert same_bits(full, full0)
        ref = oracle_fields(streams, 721, 1440)
        assert np.array_equal(full, ref)
        check_windows(ctx, streams, full, ref, windows_of(721, 1440, 60))


@pytest.mark.parametrize("mode,err", F.LARGE_MODES, ids=["abs", "rel"])
@pytest.mark.parametrize("batch", sorted(F.LARGE_BATCHES))
def test_large_frames(batch, mode, err):
    (h, w), specs = F.LARGE_BATCHES[batch]
    fixture = json.load(open(os.path.join(L.GOLDEN, "large_frames.json")))
    frames = np.stack([F.large_frame(k, h, w, seed) for k, seed in specs])
    cfg = L.make_config((1, h, w), base_cr=fixture["base_cr"], error=err, residual_type=mode)
    with L.Context(len(frames), h, w) as ctx:
        streams = ctx.encode_frames(frames, cfg)
        full = ctx.decode_frames(streams)
        for f, spec in enumerate(specs):
            c = fixture["cases"][F.large_key(batch, spec, mode)]
            assert sha(streams[f]) == c["stream_sha256"] and sha(full[f].tobytes()) == c["decoded_sha256"], spec
        check_windows(ctx, streams, full, oracle_fields(streams, h, w), windows_of(h, w, 30))


# ---- 6. the other entry points -----------------------------------------------------------------------------------------------
ENTRY_WINDOWS = [(0, 0, 721, 1440), (300, 700, 128, 256), (0, 0, 1, 1), (720, 1439, 1, 1), (63, 127, 130, 129), (359, 0, 3, 1440), (0, 719, 721, 2),
                 (180, 360, 360, 720)]


@pytest.mark.parametrize("mode,err", ERA5_MODES, ids=["abs", "rel"])
def test_shard_and_host_entry_points(mode, err):
    """a context of 7 frames for the 24-frame batch: four batches, the second engine set"""
    streams, full = era5_batch(mode, err)
    with L.Context(7, 721, 1440) as ctx:
        assert same_bits(ctx.decode_frames(streams, shard=True), full)
        rc, _ = raw_window(ctx, streams, ENTRY_WINDOWS[1])                 # (more frames than the context holds: the one-batch call refuses)
        assert rc == 1
        for win in ENTRY_WINDOWS:
            assert same_bits(window(ctx, streams, win, "ebcc_hip_decode_shard_window"), crop(full, win)), ("shard", win)
            assert same_bits(host_window(ctx, streams, win), crop(full, win)), ("host", win)
        assert same_bits(ctx.decode_frames(streams, shard=True), full)


def test_batch_codec_window():
    from ebcc_amd import h5_batch
    streams, full = era5_batch(*ERA5_MODES[0])
    with h5_batch.BatchCodec(721, 1440, max_frames=7) as codec:
        assert same_bits(codec.decode(streams), full)                     # (defaults: today's behaviour)
        for win in ENTRY_WINDOWS:
            got = codec.decode(streams, window=win)
            assert got.shape == (len(streams), win[2], win[3]) and same_bits(got, crop(full, win)), win
        into = np.full((len(streams), 128, 256), -1.0, np.float32)
        assert codec.decode(streams, out=into, window=ENTRY_WINDOWS[1]) is into and same_bits(into, crop(full, ENTRY_WINDOWS[1]))
        for bad in [(0, 0, 0, 5), (700, 0, 22, 5), (0, 1440, 1, 1), (-1, 0, 2, 2)]:
            with pytest.raises(ValueError):
                codec.decode(streams, window=bad)


def test_read_frames_rows_cols(tmp_path):
    """h5_batch.read_frames(rows=, cols=) under an interpreter with h5py, as tests/test_hdf5_gpu.py drives the HDF5 path"""
    if not os.path.exists(CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([CONDA_PY, os.path.join(L.ROOT, "tests", "h5_window_read.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 3, r.stdout


# ---- 7. invalid windows: return value 1, a message, nothing written (raw_window checks the whole buffer) ---------------------
def test_invalid_windows_are_refused_and_write_nothing():
    names = [n for n, c in sorted(STREAMS.items()) if (c["h"], c["w"]) == (100, 130)][:5]
    streams = [bytes.fromhex(STREAMS[n]["stream_hex"]) for n in names]
    big = (1 << 64) - 1
    with L.Context(len(streams), 100, 130) as ctx:
        for entry in ("ebcc_hip_decode_frames_window", "ebcc_hip_decode_shard_window"):
            for win in [(0, 0, 0, 130), (0, 0, 100, 0), (100, 0, 1, 1), (0, 130, 1, 1), (1, 0, 100, 130), (0, 1, 100, 130), (99, 129, 2, 1),
                        (big, 0, 2, 1), (0, big, 1, 2), (2, 0, big - 1, 1), (0, 2, 1, big - 1)]:
                rc, _ = raw_window(ctx, streams, win, entry)
                assert rc == 1, (entry, win)
                assert L.product().ebcc_hip_last_error(), (entry, win)
        keep, ptrs, sizes = _args(streams)
        out = np.full(64, np.float32(3.5), np.float32)
        assert lib().ebcc_hip_decode_host_frames_window(ctx.ptr, ptrs, sizes, len(streams), 0, 0, 101, 1, out.ctypes.data) == 1
        assert (out == np.float32(3.5)).all()
        full = ctx.decode_frames(streams)                                 # the context still works
        assert same_bits(window(ctx, streams, (99, 129, 1, 1)), crop(full, (99, 129, 1, 1)))


# ---- 8. workspace independence -----------------------------------------------------------------------------------------------
def _poisoned_child(mode, err, want_sha):
    """(in the child) the 721 x 1440 batch of case 5 on poisoned workspace: full decode as the parent's, windows as its crops"""
    streams, full = era5_batch(mode, err)
    assert sha(full.tobytes()) == want_sha, "full decode differs from the parent's"
    rng = np.random.default_rng(77)
    wins = P.catalogue(721, 1440, rng)[:24] + P.random_windows(721, 1440, rng, 30) + ENTRY_WINDOWS
    with L.Context(ERA5_FRAMES, 721, 1440) as ctx:
        for win in wins:                                                  # (windows first: nothing has filled the workspace yet)
            assert same_bits(window(ctx, streams, win), crop(full, win)), win
        assert same_bits(ctx.decode_frames(streams), full)
    with L.Context(7, 721, 1440) as ctx:
        for win in ENTRY_WINDOWS[:4]:
            assert same_bits(window(ctx, streams, win, "ebcc_hip_decode_shard_window"), crop(full, win)), ("shard", win)
            assert same_bits(host_window(ctx, streams, win), crop(full, win)), ("host", win)
    print("WINDOW_CHILD ok", flush=True)


@pytest.mark.parametrize("pattern", ["0xFF", "0x7F"])
def test_poisoned_workspace(pattern):
    mode, err = ERA5_MODES[0]
    _, full = era5_batch(mode, err)
    env = {k: v for k, v in os.environ.items() if not k.startswith("EBCC_")}
    env["EBCC_HIP_POISON_ALLOC"] = pattern
    code = (f"import sys; sys.path.insert(0, {L.ROOT!r}); from tests import test_window_gpu as T; "
            f"T._poisoned_child({mode!r}, {err!r}, {sha(full.tobytes())!r})")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=L.ROOT, timeout=900)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-1500:]}{r.stderr[-3000:]}"
    assert "WINDOW_CHILD ok" in r.stdout


# ---- 9. no state left behind -------------------------------------------------------------------------------------------------
def test_sequence_on_one_context_equals_fresh_contexts():
    names = [n for n, c in sorted(STREAMS.items()) if (c["h"], c["w"]) == (100, 130)]
    a, b = names[:9], names[20:33]
    sa, sb = ([bytes.fromhex(STREAMS[n]["stream_hex"]) for n in part] for part in (a, b))
    w1, w2, w3 = (10, 20, 50, 70), (63, 64, 37, 66), (0, 0, 100, 130)

    def fresh(fn):
        with L.Context(16, 100, 130) as c:
            return fn(c)

    def golden(fields, part):
        for n, d in zip(part, fields):
            assert sha(d.tobytes()) == STREAMS[n]["decoded_sha256"], n

    with L.Context(16, 100, 130) as ctx:
        steps = [("window A", lambda c: window(c, sa, w1)), ("full A", lambda c: c.decode_frames(sa)), ("other window A", lambda c: window(c, sa, w2)),
                 ("window B", lambda c: window(c, sb, w1)), ("full B", lambda c: c.decode_frames(sb)), ("whole-frame window B", lambda c: window(c, sb, w3)),
                 ("full A again", lambda c: c.decode_frames(sa))]
        for what, fn in steps:
            got = fn(ctx)
            assert same_bits(got, fresh(fn)), what
            if what.startswith("full"):
                golden(got, a if " A" in what else b)


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def test_truncated_codestream_is_refused_like_the_full_decode():
    names = [n for n, c in sorted(STREAMS.items()) if (c["h"], c["w"]) == (100, 130) and c["mode"] == L.MAX_ERROR][:4]
    streams = [bytes.fromhex(STREAMS[n]["stream_hex"]) for n in names]
    s = streams[2]
    tail = struct.unpack("<Q", s[40:48])[0]
    cut = 40
    assert tail > 200
    streams[2] = s[:40] + struct.pack("<Q", tail - cut) + s[48:len(s) - cut]            # a consistent header over a codestream that ends early
    with L.Context(4, 100, 130) as ctx:
        keep, ptrs, sizes = _args(streams)
        out = L.DeviceArray(nbytes=4 * 100 * 130 * 4)
        assert L.product().ebcc_hip_decode_frames(ctx.ptr, ptrs, sizes, 4, out.ptr) != 0
        out.free()
        for entry in ("ebcc_hip_decode_frames_window", "ebcc_hip_decode_shard_window"):
            rc, _ = raw_window(ctx, streams, (10, 10, 30, 30), entry)
            assert rc != 0, entry
        good = [bytes.fromhex(STREAMS[n]["stream_hex"]) for n in names]
        assert same_bits(window(ctx, good, (10, 10, 30, 30)), crop(ctx.decode_frames(good), (10, 10, 30, 30)))
