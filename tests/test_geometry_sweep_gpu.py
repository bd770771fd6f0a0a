"""GPU: every stage of the codec, bit for bit against the live oracle, over the frame-geometry catalogue of tests/_geometry.py
(the CPU module tests/test_geometry_sweep.py shows what the catalogue covers and holds the oracle to the reference on it).

The other modules pin the stages densely in content and at a dozen frame sizes; here the content is plain and the sizes are
chosen for what they make the wavelet kernels do: which of the five 9/7 levels have an odd extent (the boundary forms of the
lifting steps), the residual layer's pad and crop, where the frame ends in a strip of the fused inverse levels, how many
vertical pieces a level is cut into, the one-column coarsest band, and the parity of a chunk's second tile at every level.

Parts: the JPEG 2000 stages (tables, codestreams, decode, emulated decode), the residual stages (coefficients, streams, decodes,
prefix reconstructions), the probes of the truncation search (ebcc_hip_spiht_decode_prefix takes the separate passes; the strip
and piece kernels k_finest_inv_use and k_level_inv_fused are reached through ebcc_hip_residual_probe), the whole codec with
windows at the frame's last rows and columns, and chunks of two frames.

One id per shape and part of the codec; a failure names the shape, the stage, the frame and the first differing sample.
Everything is compared as bit patterns."""
import numpy as np
import pytest

from tests import _geometry as G
from tests import _j2k_tables as T
from tests import _lib as L
from tests import _probes as P
from tests.test_codec_gpu import api_decode, api_encode
from tests.test_probe_residual_gpu import designed_budget
from tests.test_window_gpu import crop, raw_window

pytestmark = pytest.mark.gpu

EMU_TARGETS = [0.5 / 65535, 0.01, 0.05, 0.1, 0.3, 1.0]
PREFIX_FRACTIONS = (1.0, 0.33, 0.07)


def same(got, want, what):
    d = T.first_difference(got, want)
    assert d is None, f"{what}: {d}"


def same_bytes(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} bytes against the oracle's {len(want)}"
    same(np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8), what + ": byte")


@pytest.fixture
def plain_env(monkeypatch):
    for k in G.ENV + ("EBCC_T1_TWO_PHASE", "EBCC_HIP_SYM_ROWS", "EBCC_T1_LPW", "EBCC_T1_DEC_TIERS"):
        monkeypatch.delenv(k, raising=False)
    L.oracle().orc_set_j2k_backend(0)


# ---- JPEG 2000 stages
@pytest.mark.parametrize("shape", G.PLAIN, ids=G.shape_id)
def test_j2k_stages(shape, plain_env):
    h, w = shape
    at = f"{h}x{w} (family {G.family(shape)})"
    frames = G.j2k_frames(h, w)
    n = len(frames) * len(G.J2K_RATES)
    batch = np.repeat(frames, len(G.J2K_RATES), axis=0)                   # frame k at rate k % 2
    rates = list(G.J2K_RATES) * len(frames)
    kinds = [k for k in G.J2K_KINDS for _ in G.J2K_RATES]
    want_streams, want_fields, mms = [], [], []
    for x, cr in zip(batch, rates):
        u16, mn, mx = L.scale_u16(x)
        s = L.orc_j2k_encode(u16, cr)
        want_streams.append(s)
        want_fields.append(L.map_decoded(L.orc_j2k_decode(s), mn, mx))
        mms.append((mn, mx))
    with L.Context(n, h, w) as ctx:
        # forward: the tile buffer's coefficients, Q6 and the tier-1 tables against the oracle's sinks, code-block by code-block
        t = ctx.j2k_tables(frames)
        assert t.retried == 0
        for f, kind in enumerate(G.J2K_KINDS):
            assert np.array_equal(T.frame(kind, h, w), frames[f]), kind
            assert t.const[f] == 0, f"{at}: frame {f} ({kind}) is flagged constant"
            assert T.compare_frame(t, f, kind) > 0
        # codestreams
        got, mm, d = ctx.j2k_encode(batch, rates, keep_device=True)
        emu, nbad, esum = ctx.j2k_emulated_decode(d, n, EMU_TARGETS)
        d.free()
        dec = ctx.j2k_decode(want_streams, mms)
    for f in range(n):
        who = f"{at} frame {f} ({kinds[f]}) cr {rates[f]:g}"
        assert (mm[f, 0], mm[f, 1]) == mms[f], f"range: {who}"
        same_bytes(got[f], want_streams[f], f"codestream: {who}")
        same(dec[f], want_fields[f], f"decode: {who}: sample (y, x)")
        same(emu[f], want_fields[f], f"emulated decode: {who}: sample (y, x)")
        err = batch[f] - want_fields[f]
        assert int(nbad[f]) == int((np.abs(err) > np.float32(EMU_TARGETS[f])).sum()), f"emulated decode: nbad: {who}"
        assert abs(esum[f] - err.astype(np.float64).sum()) <= 1e-6 * max(1.0, abs(esum[f])), f"emulated decode: esum: {who}"


# ---- residual stages
@pytest.mark.parametrize("shape", G.PLAIN, ids=G.shape_id)
def test_residual_stages(shape, plain_env):
    h, w = shape
    at = f"{h}x{w} (family {G.family(shape)})"
    imgs = G.residual_frames(h, w)
    n = len(imgs)
    budgets = G.spiht_budgets(h, w)
    want = {tb: [L.orc_spiht_encode(x, tb) for x in imgs] for tb in budgets}
    with L.Context(n * len(budgets), h, w) as ctx:
        c, dc = ctx.spiht_coeffs(imgs)
        for f, x in enumerate(imgs):
            ref, rdc = L.orc_spiht_coeffs(x)
            who = f"{at} frame {f} ({G.RESIDUAL_KINDS[f]})"
            assert dc[f] == rdc, f"DC: {who}: {dc[f]} against {rdc}"
            same(c[f].reshape(ref.shape), ref, f"coefficients (forward 9/7 of the padded frame): {who}: sample (y, x)")
        for tb in budgets:
            got = ctx.spiht_encode(imgs, [tb] * n)
            for f in range(n):
                same_bytes(got[f], want[tb][f], f"stream: {at} frame {f} ({G.RESIDUAL_KINDS[f]}) trunc_bits {tb}")
        # the decoder on the oracle's streams, whole and cut to a third
        streams = [s for tb in budgets for s in want[tb]]
        cuts = [s[:G.third(s)] for s in streams]
        full, part = ctx.spiht_decode(streams), ctx.spiht_decode(cuts)
        for k, s in enumerate(streams):
            who = f"{at} frame {k % n} ({G.RESIDUAL_KINDS[k % n]}) trunc_bits {budgets[k // n]}"
            same(full[k], L.orc_spiht_decode(s, h, w), f"decode: {who}: sample (y, x)")
            same(part[k], L.orc_spiht_decode(cuts[k], h, w), f"decode of a third: {who}: sample (y, x)")
        # the prefix reconstruction (the encoder's bookkeeping through launch_reconstruct and the separate passes; the strip and
        # piece kernels are test_truncation_probes' business) against a decode of the prefix
        tb = budgets[1]
        streams = ctx.spiht_encode(imgs, [tb] * n)
        for frac in PREFIX_FRACTIONS:
            nbytes = [max(17, int(len(s) * frac)) for s in streams]
            got = ctx.spiht_decode_prefix(n, [8 * m for m in nbytes])
            for f, s in enumerate(streams):
                same(got[f], L.orc_spiht_decode(s[:nbytes[f]], h, w, 8 * nbytes[f]),
                     f"prefix reconstruction: {at} frame {f} ({G.RESIDUAL_KINDS[f]}) fraction {frac}: sample (y, x)")


# ---- the probes of the truncation search: the strip and piece kernels of the residual layer's inverse (k_finest_inv_use,
#      k_level_inv_fused), which report statistics of a decode they never perform and write no field
@pytest.mark.parametrize("shape", G.PLAIN, ids=G.shape_id)
def test_truncation_probes(shape, plain_env):
    """x the era5-like frame, d = x - r for the three residual frames r: maximum error bit for bit and the error sum within
    the bound of a double sum taken in any order (tests/_probes.py), at five cuts, in both forms of the probe"""
    h, w = shape
    at = f"{h}x{w} (family {G.family(shape)})"
    x = G.codec_frame(h, w)
    rs = G.residual_frames(h, w)
    n = len(rs)
    xs = np.ascontiguousarray(np.stack([x] * n))
    ds = np.ascontiguousarray((xs - rs).astype(np.float32))
    res = [P.Residual(xs[f], ds[f], designed_budget(h, w)) for f in range(n)]
    cuts = [[len(r.stream), max(17, 2 * len(r.stream) // 3), max(17, len(r.stream) // 3), max(17, int(0.07 * len(r.stream))), 17] for r in res]
    with L.Context(n, h, w) as ctx:
        bx, bd = L.DeviceArray(xs), L.DeviceArray(ds)
        rmin, rmax, _, streams = ctx.residual_prepare(bx, bd, n, [designed_budget(h, w)] * n)
        for f in range(n):
            who = f"{at} frame {f} ({G.RESIDUAL_KINDS[f]})"
            assert (P.f32_bits(rmin[f]), P.f32_bits(rmax[f])) == (P.f32_bits(res[f].rmin), P.f32_bits(res[f].rmax)), f"residual range: {who}"
            same_bytes(streams[f], res[f].stream, f"residual stream: {who}")
        got = {"frames": [ctx.residual_probe(bx, bd, n, list(range(n)), [8 * cuts[f][j] for f in range(n)]) for j in range(5)]}
        frame_of = [f for j in range(5) for f in range(n)]
        bits, sums = ctx.residual_probe(bx, bd, n, frame_of, [8 * cuts[f][j] for j in range(5) for f in range(n)], slots=True)
        got["slots"] = [(bits[j * n:(j + 1) * n], sums[j * n:(j + 1) * n]) for j in range(5)]
        bx.free()
        bd.free()
    for form, rounds in got.items():
        for j, (b, s) in enumerate(rounds):
            for f in range(n):
                wb, ws, bound = res[f].stats(cuts[f][j])
                who = f"{at} frame {f} ({G.RESIDUAL_KINDS[f]}) cut of {cuts[f][j]} bytes, {form} form"
                assert int(b[f]) == wb, f"probe maximum: {who}: {int(b[f]):#x} against {wb:#x}"
                assert abs(float(s[f]) - ws) <= bound, f"probe sum: {who}: {float(s[f])!r} against {ws!r} (bound {bound!r})"


# ---- the whole codec, and windows at the frame's last rows and columns
def windows_of(h, w):
    wins = [(0, w - 3, h, 3), (h - 3, 0, 3, w), (h - 3, w - 3, 3, 3)]
    if w > 120:
        wins.append((0, 118, h, min(5, w - 118)))                        # columns 118 .. 122 (as far as the frame has them): across the first strip's edge
    return wins + [(0, 0, h, w)]


@pytest.mark.parametrize("shape", G.PLAIN, ids=G.shape_id)
def test_whole_codec_and_windows(shape, plain_env):
    h, w = shape
    at = f"{h}x{w} (family {G.family(shape)})"
    x = G.codec_frame(h, w)
    cfgs = [G.codec_config((1, h, w), x, mode) for _, mode in G.CODEC_MODES]
    want = [L.orc_encode(x, cfg) for cfg in cfgs]
    fields = np.stack([L.orc_decode(s).reshape(h, w) for s in want])
    with L.Context(len(cfgs), h, w) as ctx:
        for (name, _), cfg, s in zip(G.CODEC_MODES, cfgs, want):
            assert s, f"{at} {name}: the oracle wrote no stream"
            same_bytes(ctx.encode_frames(x[None], cfg)[0], s, f"encode: {at} {name}")
        full = ctx.decode_frames(want)
        for k, (name, _) in enumerate(G.CODEC_MODES):
            same(full[k], fields[k], f"decode: {at} {name}: sample (y, x)")
        for win in windows_of(h, w):
            rc, got = raw_window(ctx, want, win)
            if rc and w == 32:
                # documented: a window is written by the fused top level, and a geometry without one is refused
                assert b"no fused top level" in L.product().ebcc_hip_last_error(), L.product().ebcc_hip_last_error()
                continue
            assert rc == 0, (at, win, L.product().ebcc_hip_last_error())
            for k, (name, _) in enumerate(G.CODEC_MODES):
                same(got[k], np.ascontiguousarray(crop(full, win)[k]), f"window {win}: {at} {name}: sample (y, x) of the window")


# ---- chunks of two frames: the second tile at every row offset mod 32
@pytest.mark.parametrize("shape", G.D, ids=G.shape_id)
def test_chunks(shape, plain_env):
    f, h, w = shape
    at = G.shape_id(shape)
    x = G.chunk_frames(f, h, w)
    u16 = L.scale_u16(x)[0]
    with L.Context(f, h, w, tiles=f) as ctx:
        t = ctx.j2k_tables(x)
    assert t.retried == 0
    for k in range(f):
        want = L.orc_j2k_analysis(u16, k)
        label = f"era5_like tile {k}"
        assert t.const[k] == 0 and T.own_blocks(t, k, k) == len(want) > 0, (at, k, len(want))
        for stage in T.STAGES:
            for b in range(len(want)):
                T.compare_block(t, k, b, want[b], label, (stage,), k)
    cfg = G.chunk_config(shape, x)
    want = L.orc_encode(x, cfg)
    assert want, f"{at}: the oracle wrote no stream"
    got = api_encode(x, cfg)
    same_bytes(got, want, f"chunk stream: {at}")
    same(api_decode(got).reshape(f, h, w), L.orc_decode(want).reshape(f, h, w), f"chunk decode: {at}: sample (tile, y, x)")
