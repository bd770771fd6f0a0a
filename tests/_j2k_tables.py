"""The rate-independent tables of the JPEG 2000 encoder - forward 9/7 coefficients, Q6, tier-1 with its per-pass byte
counts, the distortion sums - as ebcc_hip_j2k_tables returns them, against the oracle's analysis of the same frame
(tests/_lib.py: orc_j2k_analysis), code-block by code-block.  Every comparison is exact: integers as integers, floats and
doubles by bit pattern.  A mismatch names the stage, the shape, the frame, the code-block (band, rectangle) and the first
pass or sample that differs (tests/test_j2k_tables_gpu.py)."""
import functools
import time

import numpy as np

from tests import _fields as F
from tests import _lib as L

ORIENT = ("LL", "HL", "LH", "HH")
BATCH = ("era5_like", "noise", "constant", "spike", "checker", "era5_like")
# stages in the order the encoder produces them, so that the first one reported is the first one that departs
STAGES = ("geometry", "coefficients", "Q6", "numbps", "totalpasses", "len", "rates", "disto", "bytes")
ORACLE_SECONDS = 0.1                                                    # the oracle's analysis of one frame stays under this


@functools.lru_cache(maxsize=None)
def frame(kind, h, w):
    if kind == "era5_like":
        return L.era5_like(h, w, h + w)
    if kind == "constant":
        return np.full((h, w), 273.15, np.float32)
    return F.field(kind, h, w)


def batch(h, w, kinds=BATCH):
    return np.stack([frame(k, h, w) for k in kinds])


@functools.lru_cache(maxsize=None)
def oracle_blocks(kind, h, w):
    """the oracle's code-blocks of L.scale_u16 of the frame (computed once, shared, never written to) and the CPU seconds
    the analysis took (the least of up to three runs, the later ones made only if the first is not under ORACLE_SECONDS)"""
    u16 = L.scale_u16(frame(kind, h, w))[0]
    t0 = time.process_time()
    blocks = L.orc_j2k_analysis(u16)
    seconds = time.process_time() - t0
    for _ in range(2):
        if seconds < ORACLE_SECONDS:
            break
        t0 = time.process_time()
        L.orc_j2k_analysis(u16)
        seconds = min(seconds, time.process_time() - t0)
    for b in blocks:
        for k in ("q", "cf", "rates", "disto"):
            b[k].setflags(write=False)
    return tuple(blocks), seconds


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def where(t, f, b, kind):
    k = t.blocks[f, b]
    return (f"{t.h}x{t.w} frame {f} ({kind}) code-block {b}: resolution {k['res']} {ORIENT[k['orient']]}, "
            f"{k['w']}x{k['h']} at x={k['x']} y={k['y']}")


def first_difference(got, want):
    """None, or a description of the first element at which two arrays differ (by bit pattern for floats)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    bad = np.argwhere(bits(got) != bits(want))
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    g, w_ = got[i], want[i]
    if got.dtype.kind == "f":
        return f"first at {i}: {g!r} ({int(bits(got)[i]):#x}) against {w_!r} ({int(bits(want)[i]):#x}); {len(bad)} of {got.size} differ"
    return f"first at {i}: {int(g)} against {int(w_)}; {len(bad)} of {got.size} differ"


def compare_block(t, f, b, want, kind, stages=STAGES):
    """code-block b of frame f of the tables t against the oracle's code-block `want`, stage by stage"""
    k = t.blocks[f, b]
    at = where(t, f, b, kind)
    for stage in stages:
        if stage == "geometry":
            got, ref = (int(k["w"]), int(k["h"]), int(k["orient"])), (want["w"], want["h"], want["orient"])
            assert got == ref, f"geometry: {at}: (w, h, orient) {got} against the oracle's {ref}"
            assert 0 <= k["x"] and k["x"] + k["w"] <= t.w and 0 <= k["y"] and k["y"] + k["h"] <= t.h, f"geometry: {at}: outside the frame"
        elif stage == "coefficients":
            d = first_difference(t.rect(t.coeffs, f, b), want["cf"])
            assert d is None, f"coefficients (forward 9/7): {at}: sample (y, x) {d}"
        elif stage == "Q6":
            d = first_difference(t.rect(t.q6, f, b), want["q"])
            assert d is None, f"Q6 (quantisation, six fractional bits): {at}: sample (y, x) {d}"
        elif stage in ("numbps", "totalpasses", "len"):
            assert int(k[stage]) == want[stage], f"{stage} (tier-1): {at}: {int(k[stage])} against {want[stage]}"
        elif stage == "rates":
            d = first_difference(t.passes(f, b)[0], want["rates"])
            assert d is None, f"rates (tier-1 bytes per pass): {at}: pass {d}"
        elif stage == "disto":
            d = first_difference(t.passes(f, b)[1], want["disto"])
            assert d is None, f"disto (k_distortion): {at}: pass {d}"
        elif stage == "bytes":
            got, ref = t.block_bytes(f, b), want["bytes"]
            d = first_difference(np.frombuffer(got, np.uint8), np.frombuffer(ref, np.uint8))
            assert d is None, f"bytes (tier-1): {at}: byte {d}"
        else:
            raise KeyError(stage)


def compare_frame(t, f, kind, stages=STAGES):
    """every code-block of frame f against the oracle; returns the number compared"""
    want, _ = oracle_blocks(kind, t.h, t.w)
    assert len(want) == t.nblocks, f"{t.h}x{t.w}: {t.nblocks} code-blocks a frame against the oracle's {len(want)}"
    # stage-major: the report is the earliest stage that departs anywhere in the frame, not the first code-block's latest
    for stage in stages:
        for b in range(t.nblocks):
            compare_block(t, f, b, want[b], kind, (stage,))
    return len(want)


def same_tables(a, fa, b, fb, what, coeffs=True):
    """frame fa of tables a and frame fb of tables b hold the same bits"""
    assert a.nblocks == b.nblocks
    if coeffs:
        d = first_difference(a.coeffs[fa], b.coeffs[fb])
        assert d is None, f"{what}: coefficients: {d}"
    d = first_difference(a.q6[fa], b.q6[fb])
    assert d is None, f"{what}: Q6: {d}"
    for i in range(a.nblocks):
        ka, kb = a.blocks[fa, i], b.blocks[fb, i]
        for name in ("x", "y", "w", "h", "orient", "res", "numbps", "totalpasses", "len"):
            assert ka[name] == kb[name], f"{what}: code-block {i}: {name} {ka[name]} against {kb[name]}"
        for j, stage in enumerate(("rates", "disto")):
            d = first_difference(a.passes(fa, i)[j], b.passes(fb, i)[j])
            assert d is None, f"{what}: code-block {i}: {stage}: pass {d}"
        assert a.block_bytes(fa, i) == b.block_bytes(fb, i), f"{what}: code-block {i}: bytes"


def constant_frame_is_left_out(t, f):
    assert t.const[f] == 1, f"frame {f} is not flagged constant"
    k = t.blocks[f]
    assert not k["numbps"].any() and not k["totalpasses"].any() and not k["len"].any(), f"frame {f}: a constant frame has coded code-blocks"
