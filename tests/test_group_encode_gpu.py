"""GPU: frame groups (ebcc_hip_encode_frames_groups / _shard_groups / _host_frames_groups, ebcc_hip_group_ranges,
include/ebcc_hip.h; ebcc_amd/h5_batch.py: BatchCodec.encode_groups, write_variables).  Every comparison is bitwise and the
yardstick is the oracle, which is pinned to the reference build: frame f of a group is the oracle's ebcc_encode of that
frame with the group's config, a group with range_of_group is the oracle's ebcc_encode_chunking_compat of the group in
one-frame chunks, and nothing depends on how groups, batches, slices and engine sets cut the frames.

Twelve frames of 70 x 100 in four groups: G0 frames 0-2 NONE at rate 15, G1 frames 3-6 MAX_ERROR 0.02 at 30 (frame 4
constant, frame 5 nearly flat), G2 frames 7-8 RELATIVE_ERROR 0.002 of the frame's own range at 8, G3 frames 9-11
RELATIVE_ERROR 0.002 of the group's range at 15 (frame 10 has three times the range of its neighbours).  The first test asserts
on the oracle's own output what the cases are: with the default environment every searching frame ends on the pure base layer
(search #2 and the comparison of src/ebcc_codec.c:838), with EBCC_INIT_BASE_ERROR_QUANTILE=0.02 and the fallback disabled they
keep their residual layers, and in both G3's compat chunks differ from the streams of the per-frame range - so a pass can come
neither from one config for all frames nor from the wrong range."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import _lib as L

pytestmark = pytest.mark.gpu

H, W, N = 70, 100, 12
SENT = np.uint32(0xA5A5A5A5)
FRONT, BACK = 64, 37                                  # floats of sentinel before (256 bytes) and behind
#          first, count, mode, error, base_cr, range_of_group
GROUPS = [(0, 3, L.NONE, 0.0, 15.0, 0), (3, 4, L.MAX_ERROR, 0.02, 30.0, 0), (7, 2, L.RELATIVE_ERROR, 0.002, 8.0, 0),
          (9, 3, L.RELATIVE_ERROR, 0.002, 15.0, 1)]
ENVS = {"default": {}, "residual": {"EBCC_INIT_BASE_ERROR_QUANTILE": "0.02", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK": "1"}}
KINDS = {"default": "bbb" "bcbb" "bb" "bbb", "residual": "bbb" "rcbr" "rr" "rrr"}
CONDA_PY = "/opt/conda/bin/python3.9"


class FrameGroup(ctypes.Structure):
    """ebcc_hip_frame_group"""
    _fields_ = [("frames", ctypes.c_void_p), ("n_frames", ctypes.c_size_t), ("config", L.CodecConfig), ("range_of_group", ctypes.c_int)]


def lib():
    """the product with the new entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = L.product()
    group_p = ctypes.POINTER(FrameGroup)
    for name in ("ebcc_hip_encode_frames_groups", "ebcc_hip_encode_shard_groups", "ebcc_hip_encode_host_frames_groups"):
        fn = getattr(p, name)
        fn.argtypes, fn.restype = [ctypes.c_void_p, group_p, ctypes.c_size_t, L.c_void_pp, L.c_size_p], ctypes.c_int
    p.ebcc_hip_group_ranges.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    p.ebcc_hip_group_ranges.restype = ctypes.c_int
    return p


def error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


@pytest.fixture(autouse=True)
def _entry_points():
    lib()                                                                 # every test of this file needs them


def use_env(monkeypatch, env):
    for name in ENVS["residual"]:
        monkeypatch.delenv(name, raising=False)
    for name, value in ENVS[env].items():
        monkeypatch.setenv(name, value)
    L.oracle().orc_set_j2k_backend(0)


# ---- inputs and the oracle's streams, made once ---------------------------------------------------------------------------------
_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def frames():
    def make():
        a = np.stack([L.era5_like(H, W, 20 + i, 1.0 + 0.1 * (i % 4), 0.6) for i in range(N)])
        a = (a + 0.05 * np.arange(W)[None, None, :] + 0.03 * np.arange(H)[None, :, None]).astype(np.float32)
        a[4] = 7.0
        a[5] = 250 + (a[5] - 250) * np.float32(1e-4)
        a[10] = (a[10] - 250) * np.float32(3) + 250
        a.setflags(write=False)
        return a
    return once("frames", make)


def frame_config(mode, err, base_cr):
    return L.make_config((1, H, W), base_cr=base_cr, error=err, residual_type=mode)


def entries(buf):
    """the chunk streams of a container"""
    out, p = [], 80
    while p < len(buf):
        n = struct.unpack("<Q", buf[p:p + 8])[0]
        out.append(buf[p + 8:p + 8 + n])
        p += 8 + n
    return out


def kinds(streams):
    """c: constant frame, b: base layer alone, r: with a residual layer"""
    heads = [struct.unpack("<4sBBHIIQIIQQ", s[:48]) for s in streams]
    return "".join("c" if h[2] & 1 else "b" if h[9] == 0 else "r" for h in heads)


def oracle_streams(env):
    """the twelve streams the groups must give under the environment `env` (the caller has set it)"""
    def make():
        a, out = frames(), []
        for first, count, mode, err, cr, whole in GROUPS:
            if whole:
                cfg = L.make_config((count, H, W), (1, H, W), base_cr=cr, error=err, residual_type=mode)
                out += entries(L.orc_encode(a[first:first + count], cfg, "orc_ebcc_encode_chunking_compat"))
            else:
                out += [L.orc_encode(a[f], frame_config(mode, err, cr)) for f in range(first, first + count)]
        assert len(out) == N and all(out)
        return out
    return once(("oracle", env), make)


def oracle_decodes(env):
    return once(("decoded", env), lambda: np.stack([L.orc_decode(s).reshape(H, W) for s in oracle_streams(env)]))


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


def table(items):
    """items: (pointer, frames, config, range_of_group) per group"""
    t = (FrameGroup * max(1, len(items)))()
    for g, (ptr, n, cfg, whole) in enumerate(items):
        t[g].frames, t[g].n_frames, t[g].config, t[g].range_of_group = ptr, n, cfg, whole
    return t


def group_items(pointers):
    """the four groups with their frames at pointers[g]"""
    return [(pointers[g], count, frame_config(mode, err, cr), whole) for g, (_, count, mode, err, cr, whole) in enumerate(GROUPS)]


def encode_groups(form, ctx, items, total=None, n_groups=None, prefill=0):
    """-> (return value, the streams or None); after a failure every out_streams entry is NULL"""
    total = sum(it[1] for it in items) if total is None else total
    outs, sizes = (ctypes.c_void_p * max(1, total))(*([prefill] * max(1, total))), (ctypes.c_size_t * max(1, total))()
    fn = getattr(lib(), "ebcc_hip_encode_" + form + "_groups")
    rc = fn(ctx.ptr, table(items) if items is not None else None, len(items) if n_groups is None else n_groups, outs, sizes)
    if rc:
        assert all(not outs[k] for k in range(total)), "streams left behind by a call that failed"
        return rc, None
    res = [ctypes.string_at(outs[k], sizes[k]) for k in range(total)]
    for k in range(total):
        L.product().free_buffer(outs[k])
    return 0, res


def separate_arrays():
    """the four groups as four device arrays, at float offsets 1, 2, 3, 0 from a 256-byte boundary"""
    a = frames()
    return [Resident(a[first:first + count], (g + 1) % 4) for g, (first, count, *_rest) in enumerate(GROUPS)]


# ---- 0. the oracle's streams are the cases this file needs ------------------------------------------------------------------------
@pytest.mark.parametrize("env", sorted(ENVS))
def test_the_oracle_streams_are_the_cases_this_file_needs(monkeypatch, env):
    use_env(monkeypatch, env)
    got = oracle_streams(env)
    assert kinds(got) == KINDS[env]
    a = frames()
    ranges = [float(a[f].max() - a[f].min()) for f in (9, 10, 11)]
    assert [round(r, 1) for r in ranges] == [56.4, 167.8, 56.6] and round(float(a[9:12].max() - a[9:12].min()), 1) == 167.8
    own = [L.orc_encode(a[f], frame_config(L.RELATIVE_ERROR, 0.002, 15.0)) for f in (9, 10, 11)]
    assert got[9] != own[0] and got[11] != own[2]
    if env == "default":
        assert [len(s) for s in got[9:12]] == [2692, 3776, 1868] and [len(s) for s in own] == [4331, 3776, 3009]


# ---- 1. a mixed batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", sorted(ENVS))
def test_mixed_batch_is_the_oracles_frame_by_frame(monkeypatch, env):
    use_env(monkeypatch, env)
    want = oracle_streams(env)
    arrays = separate_arrays()
    with L.Context(16, H, W) as ctx:
        rc, got = encode_groups("frames", ctx, group_items([r.ptr for r in arrays]), prefill=0xDEAD)
        assert rc == 0, error()
        assert kinds(got) == KINDS[env]
        for f in range(N):
            assert got[f] == want[f], (f, kinds(got), len(got[f]), len(want[f]))
        dec = ctx.decode_frames(got)
        assert np.array_equal(dec.view(np.uint32), oracle_decodes(env).view(np.uint32))
    assert all(r.unchanged() for r in arrays)
    for r in arrays:
        r.free()


# ---- 2. cuts do not matter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", sorted(ENVS))
def test_cuts_do_not_matter(monkeypatch, env):
    use_env(monkeypatch, env)
    want = oracle_streams(env)
    a = frames()
    arrays = separate_arrays()
    whole = Resident(a, 3)
    firsts = [whole.ptr + 4 * first * H * W for first, *_rest in GROUPS]
    with L.Context(5, H, W) as small, L.Context(16, H, W) as ctx:
        # batches of 5: {G0, G1[:2]}, {G1[2:], G2, G3[:1]}, {G3[1:]} - cut inside G1 and G3, sources that are not adjacent, both sets
        rc, got = encode_groups("shard", small, group_items([r.ptr for r in arrays]))
        assert rc == 0 and got == want, ("shard", error())
        # the same batches with every batch in one run of memory
        rc, got = encode_groups("shard", small, group_items(firsts))
        assert rc == 0 and got == want, ("shard, one array", error())
        # three slices of four frames
        monkeypatch.setenv("EBCC_HIP_SLICES", "3")
        rc, got = encode_groups("frames", ctx, group_items([r.ptr for r in arrays]))
        assert rc == 0 and got == want, ("slices", error())
        monkeypatch.delenv("EBCC_HIP_SLICES")
        # one contiguous device array, four groups pointing into it: read where it lies
        rc, got = encode_groups("frames", ctx, group_items(firsts))
        assert rc == 0 and got == want, ("in place", error())
        # pageable host arrays, one per group
        hosts = [np.array(a[first:first + count]) for first, count, *_rest in GROUPS]
        for c in (small, ctx):
            rc, got = encode_groups("host_frames", c, group_items([h.ctypes.data for h in hosts]))
            assert rc == 0 and got == want, ("host", c.max_frames, error())
    assert whole.unchanged() and all(r.unchanged() for r in arrays)
    for r in arrays + [whole]:
        r.free()


# ---- 3. the uniform calls are untouched -------------------------------------------------------------------------------------------
def test_one_group_is_the_uniform_call(monkeypatch):
    use_env(monkeypatch, "residual")
    a = frames()
    src = Resident(a, 2)
    with L.Context(16, H, W) as ctx:
        for mode, err, cr in ((L.NONE, 0.0, 15.0), (L.MAX_ERROR, 0.02, 30.0), (L.RELATIVE_ERROR, 0.002, 8.0)):
            cfg = frame_config(mode, err, cr)
            uniform = ctx.encode_frames(a, cfg)
            rc, got = encode_groups("frames", ctx, [(src.ptr, N, cfg, 0)])
            assert rc == 0 and got == uniform, (mode, error())
            assert got[7] == L.orc_encode(a[7], cfg), mode
    src.free()


# ---- 4. the ranges of many groups in one launch -----------------------------------------------------------------------------------
def group_ranges(ctx, pointers, lengths):
    n = len(pointers)
    mm = np.tile(np.array([-123.0, -456.0], np.float32), n)
    flags = np.full(n, 77, np.int32)
    rc = lib().ebcc_hip_group_ranges(ctx.ptr, (ctypes.c_void_p * n)(*pointers), (ctypes.c_size_t * n)(*lengths), n, mm.ctypes.data, flags.ctypes.data)
    return rc, mm.reshape(n, 2), flags


def test_group_ranges():
    rng = np.random.default_rng(11)
    lengths = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 4097)
    groups, words, at = [], [np.full(FRONT, SENT, np.uint32)], FRONT
    for k, n in enumerate(lengths):
        for off in (0, 1, 2, 3):
            x = (rng.standard_normal(n) * 100).astype(np.float32)
            if (k + off) % 2 == 0:                                         # extremes at the first and the last float: scalar head and tail
                x[0], x[-1] = (-5000.0, 6000.0) if n > 1 else (x[0], x[0])
            if (n, off) == (7, 2):
                x[:] = np.array([-0.0, 0.0] * 4, np.float32)[:n]            # only zeros of both signs
            pad = (-at) % 64 + off                                         # the group begins `off` floats behind a 256-byte boundary
            words += [np.full(pad, SENT, np.uint32), x.view(np.uint32), np.full(5, SENT, np.uint32)]
            groups.append([at + pad, n, x])
            at += pad + n + 5
    nan_at = next(g for g, (_, n, _) in enumerate(groups) if n == 65 and groups[g][0] % 4 == 1)      # head: 3 floats to the 16-byte boundary
    inf_at = next(g for g, (_, n, _) in enumerate(groups) if n == 7 and groups[g][0] % 4 == 0)       # tail: floats 4 .. 6
    image = np.concatenate(words)
    clean = image.copy()
    image[groups[nan_at][0]] = np.array([np.nan], np.float32).view(np.uint32)[0]
    image[groups[inf_at][0] + 6] = np.array([-np.inf], np.float32).view(np.uint32)[0]
    bits = lambda v: (np.float32(v) + np.float32(0)).view(np.uint32)          # noqa: E731  (-0 -> +0)
    with L.Context(2, 32, 48) as ctx:
        for data, bad in ((clean, ()), (image, (nan_at, inf_at))):
            d = L.DeviceArray(data)
            assert d.ptr % 256 == 0
            rc, mm, flags = group_ranges(ctx, [d.ptr + 4 * at for at, _, _ in groups], [n for _, n, _ in groups])
            assert rc == (2 if bad else 0), error()
            assert flags.tolist() == [1 if g in bad else 0 for g in range(len(groups))]
            for g, (_, n, x) in enumerate(groups):
                if g in bad:
                    assert mm[g].tolist() == [-123.0, -456.0], "minmax of a group with a NaN or an Inf was written"
                else:
                    assert bits(mm[g][0]) == bits(x.min()) and bits(mm[g][1]) == bits(x.max()), (g, n, mm[g], x.min(), x.max())
            assert np.array_equal(d.get(np.uint32, data.shape), data), "the input was written"
            d.free()
        zeros = next(g for g, (at, n, _) in enumerate(groups) if n == 7 and at % 4 == 2)
        assert (groups[zeros][2] == 0).all() and np.signbit(groups[zeros][2]).any()
        # one array through ebcc_hip_array_range and as a group of one: the same words, and the same flag on a planted NaN
        array_range = lib().ebcc_hip_array_range
        array_range.argtypes, array_range.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int
        x = (rng.standard_normal(4099) * 100).astype(np.float32)
        for base in (0, 1, 2, 3):
            for planted in (None, 2050):
                y = x.copy()
                if planted is not None:
                    y[planted] = np.nan
                d = L.DeviceArray(np.concatenate([np.full(FRONT + base, SENT, np.uint32), y.view(np.uint32), np.full(BACK, SENT, np.uint32)]))
                ptr = d.ptr + 4 * (FRONT + base)
                one = np.array([-123.0, -456.0], np.float32)
                rc_one = array_range(ctx.ptr, ptr, y.size, one.ctypes.data)
                rc, mm, flags = group_ranges(ctx, [ptr], [y.size])
                assert rc_one == rc == (2 if planted else 0) and flags.tolist() == [1 if planted else 0], (base, planted, error())
                assert np.array_equal(one.view(np.uint32), mm[0].view(np.uint32)), (base, planted, one, mm)
                if planted is None:
                    assert bits(one[0]) == bits(x.min()) and bits(one[1]) == bits(x.max())
                d.free()
        d = L.DeviceArray(clean)
        assert group_ranges(ctx, [d.ptr, None], [4, 4])[0] == 1 and error()
        assert group_ranges(ctx, [d.ptr, d.ptr], [4, 0])[0] == 1 and error()
        assert group_ranges(ctx, [d.ptr + 2], [4])[0] == 1 and error()
        d.free()


# ---- 5. refusals and NaN ----------------------------------------------------------------------------------------------------------
def test_refusals_and_nan(monkeypatch):
    use_env(monkeypatch, "residual")
    want = oracle_streams("residual")
    a = frames()
    arrays = separate_arrays()
    ptrs = [r.ptr for r in arrays]
    good = group_items(ptrs)
    cfg = good[1][2]
    with L.Context(16, H, W) as ctx, L.Context(8, H, W) as eight, L.Context(16, 64, 96) as other:
        rc, _ = encode_groups("frames", eight, good, prefill=0xDEAD)                      # twelve frames, room for eight
        assert rc == 1 and error()
        for form in ("frames", "shard", "host_frames"):
            assert encode_groups(form, other, good)[0] == 1 and error(), form              # a context of another geometry
            refused = {"no groups": (good, 0), "a null list": (None, 4),
                       "a group without frames": (good[:2] + [(ptrs[2], 0, cfg, 0)], None),
                       "a group with a null pointer": ([(None, 3, cfg, 0)] + good[1:], None),
                       "dims of two frames": (good[:3] + [(ptrs[3], 3, L.make_config((2, H, W), base_cr=15.0), 0)], None),
                       "a total that overflows": ([(ptrs[0], (1 << 63) + 1, cfg, 0), (ptrs[1], (1 << 63) + 1, cfg, 0)], None)}
            for what, (items, n_groups) in refused.items():
                rc, _ = encode_groups(form, ctx, items, total=N, n_groups=n_groups)
                assert rc == 1 and error(), (form, what)
        # a NaN in G2 (the frame's own check) and in G3 (the group's range): 2, the group named, and the process goes on
        for g, frame in ((2, 8), (3, 10)):
            first, count = GROUPS[g][:2]
            x = a[first:first + count].copy()
            x[frame - first, 33, 57] = np.nan
            bad = Resident(x, 1)
            hosts = [np.array(a[f:f + c]) for f, c, *_rest in GROUPS]
            hosts[g] = x
            for form, these in (("frames", ptrs), ("shard", ptrs), ("host_frames", [h.ctypes.data for h in hosts])):
                these = list(these)
                if form != "host_frames":
                    these[g] = bad.ptr
                rc, _ = encode_groups(form, ctx, group_items(these), prefill=0xDEAD)
                assert rc == 2 and "group %d" % g in error(), (form, g, error())
            bad.free()
        rc, got = encode_groups("frames", ctx, good)
        assert rc == 0 and got == want, error()
    for r in arrays:
        r.free()


# ---- 6. Python --------------------------------------------------------------------------------------------------------------------
OPTS = {L.NONE: "none", L.MAX_ERROR: "max_error_target", L.RELATIVE_ERROR: "relative_error_target"}


def test_python_encode_groups(monkeypatch):
    use_env(monkeypatch, "residual")
    from ebcc_amd import h5_batch
    a = frames()
    with h5_batch.BatchCodec(H, W, max_frames=5) as codec:
        got = codec.encode_groups([(a[first:first + count], cr, (OPTS[mode], err if mode else None), bool(whole))
                                   for first, count, mode, err, cr, whole in GROUPS])
        assert [len(g) for g in got] == [3, 4, 2, 3]
        assert sum(got, []) == oracle_streams("residual")
        with pytest.raises(ValueError):
            codec.encode_groups([(a[:2, :60], 15.0, ("none", None))])


def test_python_write_variables(tmp_path):
    if not os.path.exists(CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([CONDA_PY, os.path.join(L.ROOT, "tests", "h5_variables.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 3, r.stdout
