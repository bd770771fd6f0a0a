"""GPU: k_spiht_decode, k_spiht_encode and k_reconstruct bit-exact against the CPU oracle at every bit budget and every cut of
tests/_spiht_cuts.py (the oracle is held to the reference build on the same catalogue by tests/test_spiht_cuts.py).

The decoder's budget code runs in the last one or two chunks of a frame only, and which of its tests fires depends on the kind
of bit the budget falls on; a frame of a decode launch is one wave, so 64 cuts cost one call.  num_bits is honoured to the bit:
each cut is decoded with just the bytes it needs (bits past the end read as 0) and with the whole stream (the bits past the
budget are real data the kernel reads ahead), and past the header's bits0.  A call mixes short and long cuts and both forms, so a
frame that stops early sits beside frames that run on, and a stream slot that held a long stream next holds a short one.
Images are compared as uint32, so -0 and +0 differ.  Every test counts its comparisons against the catalogue."""
import ctypes

import numpy as np
import pytest

from tests import _lib as L
from tests import _spiht_cuts as S

pytestmark = pytest.mark.gpu

COUNT = {"decode": 0, "decode-mixed": 0, "budget": 0, "budget-prefix": 0, "prefix": 0, "floor": 0}


def _same(got, want):
    return np.array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))


def _decode_call(ctx, h, w, frames, bad, what):
    """one ebcc_hip_spiht_decode over frames of (tag, stream, num_bits, size); the comparisons made"""
    got = ctx.spiht_decode([s[:size] for _, s, _, size in frames], [nb for _, _, nb, _ in frames])
    want = S.threaded(L.orc_spiht_decode, [(s[:size], h, w, nb) for _, s, nb, size in frames])
    for f, ref in enumerate(want):
        if not _same(got[f], ref):
            tag, _, nb, size = frames[f]
            bad.append((what, tag, nb, size, int((got[f].view(np.uint32) != ref.view(np.uint32)).sum())))
    return len(frames)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_decoder_at_every_cut(case):
    h, w, name = case
    s = S.stream(h, w, name)
    bad, made = [], 0
    with L.Context(S.PER_CALL, h, w) as ctx:
        for k, call in enumerate(S.interleaved_pairs(h, w, len(s))):
            made += _decode_call(ctx, h, w, [(name, s, nb, size) for nb, size in call], bad, k)
    COUNT["decode"] += made
    assert made == len(S.decode_pairs(h, w, len(s)))
    assert not bad, (len(bad), sorted(bad, key=lambda b: b[2:4])[:12])


@pytest.mark.parametrize("geom", S.GEOMS, ids=lambda g: "{}x{}".format(*g))
def test_decoder_batches_mix_images(geom):
    """frame i of a call is image i % 5: the per-frame bases of the lists and the per-frame state"""
    h, w = geom
    bad, made = [], 0
    with L.Context(S.PER_CALL, h, w) as ctx:
        for k, call in enumerate(S.mixed_calls(h, w)):
            assert len({name for name, _, _ in call}) == len(S.IMAGES)
            made += _decode_call(ctx, h, w, [(name, S.stream(h, w, name), nb, size) for name, nb, size in call], bad, k)
    COUNT["decode-mixed"] += made
    assert made == S.MIXED_CALLS * S.PER_CALL
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_encoder_at_every_budget(case):
    """length and bytes at every budget, and after each call the bookkeeping path at the whole stream: the first decode of the
    truncation search (src/ebcc_codec.c:749)"""
    h, w, name = case
    img = S.image(h, w, name)
    budgets = S.encode_budgets(h, w, name)
    bad, made, made_prefix = [], 0, 0
    with L.Context(S.PER_CALL, h, w) as ctx:
        for call in S.interleaved(budgets):
            n = len(call)
            got = ctx.spiht_encode(np.broadcast_to(img, (n, h, w)), call)
            want = list(S.threaded(L.orc_spiht_encode, [(img, tb) for tb in call]))
            rec = ctx.spiht_decode_prefix(n, [8 * len(e) for e in want])
            dec = S.threaded(L.orc_spiht_decode, [(e, h, w) for e in want])
            for f, ref in enumerate(dec):
                made += 1
                if len(got[f]) != len(want[f]) or got[f] != want[f]:
                    bad.append(("stream", call[f], len(got[f]), len(want[f])))
                made_prefix += 1
                if not _same(rec[f], ref):
                    bad.append(("prefix", call[f], len(want[f])))
    COUNT["budget"] += made
    COUNT["budget-prefix"] += made_prefix
    assert made == made_prefix == len(budgets)
    assert not bad, (len(bad), sorted(bad, key=lambda b: b[1])[:12])


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_prefix_reconstruction_at_every_byte(case):
    """a coefficient whose sign bit lies just past a byte cut is positive, whatever the encoder knew"""
    h, w, name = case
    s = S.stream(h, w, name)
    cuts = S.prefix_cuts(len(s))
    bad, made = [], 0
    with L.Context(S.PER_CALL, h, w) as ctx:
        got = ctx.spiht_encode(np.broadcast_to(S.image(h, w, name), (S.PER_CALL, h, w)), [S.STREAM_BITS] * S.PER_CALL)
        assert all(g == s for g in got)
        for call in S.interleaved(cuts):
            rec = ctx.spiht_decode_prefix(len(call), call)
            want = S.threaded(L.orc_spiht_decode, [(s[:c // 8], h, w, c) for c in call])
            for f, ref in enumerate(want):
                made += 1
                if not _same(rec[f], ref):
                    bad.append(call[f])
    COUNT["prefix"] += made
    assert made == len(cuts)
    assert not bad, (len(bad), sorted(bad)[:12])


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_num_bits_floor(case):
    """128 bits are the header (spiht_re.c:500-501: num_bits - 128 must be positive): refused; one bit more decodes"""
    h, w, name = case
    s = S.stream(h, w, name)
    with L.Context(1, h, w) as ctx:
        buf = ctypes.create_string_buffer(s, len(s))
        ptrs = (ctypes.c_void_p * 1)(ctypes.cast(buf, ctypes.c_void_p).value)
        out = L.DeviceArray(nbytes=h * w * 4)
        rc = ctx.lib.ebcc_hip_spiht_decode(ctx.ptr, ptrs, (ctypes.c_size_t * 1)(len(s)), (ctypes.c_size_t * 1)(128), 1, out.ptr)
        out.free()
        assert rc == 1 and ctx.lib.ebcc_hip_last_error() == b"SPIHT stream: num_bits must exceed 128"
        COUNT["floor"] += 1
        for nb, size in ((129, len(s)), (129, 17), (136, 17)):
            assert _same(ctx.spiht_decode([s[:size]], [nb])[0], L.orc_spiht_decode(s[:size], h, w, nb)), (nb, size)
            COUNT["floor"] += 1


def test_zz_comparisons_made():
    print("\nSPIHT cut comparisons: " + ", ".join(f"{k} {v}" for k, v in COUNT.items()))
    for h, w in S.GEOMS:
        d, b, p = S.totals(h, w)
        print(f"  catalogue {h}x{w}: {d} decodes (cuts x 2 sizes), {b} budgets, {p} prefix cuts, {S.MIXED_CALLS * S.PER_CALL} mixed decodes")
