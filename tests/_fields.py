"""Frames that push the entropy coders hardest, built from integer arithmetic only so that they are the same bits on
any machine (no float RNG, no FFT).  Each generator takes (h, w, seed) and returns a float32 h x w frame.

After the base layer's u16 scaling (src/ebcc_codec.c:686-689):
- noise:       white noise over the full range: every code-block at its maximum bit-plane count, the longest MQ chains;
- lowbit:      3-bit noise on a constant, two corner samples pinning the range: few bit-planes in almost every block;
- checker:     0/65535 checkerboard: every sign of the finest subbands alternates;
- spike:       one sample on zero: nearly every code-block is empty;
- edges:       steps on, and one sample beside, the 64-coefficient code-block edges of the finest subbands (image
               offsets 128k - 1, 128k, 128k + 1);
- stripes:     period-2 stripes along x: the horizontal high-pass subbands saturated, the others empty;
- smooth:      the integer formula of tests/_lib.formula_frames, the smooth control.

Every fixture made from these records the sha256 of the frame, so a platform difference in an input fails as
"input differs" rather than as a codec mismatch.
"""
import hashlib

import numpy as np

from tests import _domains as D
from tests import _lib as L


def hash32(h, w, seed):
    """A uint32 hash of (y, x, seed) (murmur3's finaliser over a mixed index), wrapping uint32 arithmetic."""
    y, x = np.mgrid[0:h, 0:w].astype(np.uint32)
    with np.errstate(over="ignore"):
        v = y * np.uint32(0x9E3779B1) ^ x * np.uint32(0x85EBCA77) ^ np.uint32((seed * 0xC2B2AE3D + 0x27D4EB2F) & 0xFFFFFFFF)
        v ^= v >> np.uint32(16)
        v *= np.uint32(0x85EBCA6B)
        v ^= v >> np.uint32(13)
        v *= np.uint32(0xC2B2AE35)
        v ^= v >> np.uint32(16)
    return v


def noise(h, w, seed):
    """24-bit white noise in [0, 1): exact in float32"""
    return ((hash32(h, w, seed) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def lowbit(h, w, seed):
    """0.5 + k / 65535 with k in 0..7, range pinned to [0, 1] by two corner samples"""
    k = (hash32(h, w, seed) & np.uint32(7)).astype(np.float32)
    a = (np.float32(0.5) + k / np.float32(65535.0)).astype(np.float32)
    a[0, 0] = 0.0
    a[-1, -1] = 1.0
    return a


def checker(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y + seed) & 1)).astype(np.float32)


def spike(h, w, seed):
    a = np.zeros((h, w), np.float32)
    a[(h // 3 + seed) % h, (w // 2 + 1 + seed) % w] = 1.0
    return a


def _step_count(n, seed):
    """for each index 0..n-1 the number of edges at or before it; edges at 128k - 1, 128k, 128k + 1 in rotation (one
    edge in the middle where the frame is too small for any)"""
    edges = [128 * k + (k + seed) % 3 - 1 for k in range(1, n // 128 + 1) if 128 * k + 1 < n] or [n // 2]
    return np.searchsorted(np.asarray(edges, np.int64), np.arange(n), side="right")


def edges(h, w, seed):
    sy = _step_count(h, seed)[:, None]
    sx = _step_count(w, seed + 1)[None, :]
    return ((sx * 7 + sy * 13 + seed) % 64).astype(np.float32)


def stripes(h, w, seed):
    x = np.arange(w)[None, :]
    return np.broadcast_to(((x + seed) & 1).astype(np.float32), (h, w)).copy()


def smooth(h, w, seed):
    return L.formula_frames(seed + 1, h, w)[seed]


KINDS = {f.__name__: f for f in (noise, lowbit, checker, spike, edges, stripes, smooth)}


def field(kind, h, w, seed=0):
    return np.ascontiguousarray(KINDS[kind](h, w, seed), np.float32)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ---- the whole codec at size (tests/test_large_frames_gpu.py, fixtures by oracle/make_golden_large.py)
LARGE_MODES = [(L.MAX_ERROR, 0.05), (L.RELATIVE_ERROR, 1e-3)]
LARGE_BASE_CR = 30.0
LARGE_BATCHES = {
    "batch_1024": ((1024, 1024), [("temperature", 1), ("precipitation", 2), ("noise", 0), ("spike", 0), ("checker", 0),
                                  ("lowbit", 0)]),
    "batch_2047": ((2047, 2047), [("mask", 3), ("noise", 1), ("spike", 2), ("edges", 0)]),
}
EXTREME_MODES = [(L.MAX_ERROR, 0.25), (L.RELATIVE_ERROR, 2e-3)]     # base_cr 40 (test_extreme_frame_sizes)
COMPAT_SHAPE = (2, 2100, 1100)


def large_frame(kind, h, w, seed):
    """a value domain of tests/_domains.py or a field of this module"""
    if kind in KINDS:
        return field(kind, h, w, seed)
    return np.ascontiguousarray(D.DOMAINS[kind](h, w, seed), np.float32)


def extreme_frame():
    return L.era5_like(2047, 2047, 11, 1.5, 2.5)


def compat_array():
    """ebcc_encode_chunking_compat's default chunks: 1024-row chunks and a 52-row edge chunk per frame"""
    h, w = COMPAT_SHAPE[1:]
    return np.ascontiguousarray(np.stack([L.formula_frames(1, h, w)[0], noise(h, w, 5) * np.float32(40.0) + np.float32(230.0)]))


def large_key(what, spec, mode):
    m = {L.MAX_ERROR: "abs", L.RELATIVE_ERROR: "rel"}[mode]
    return f"{what}-{spec[0]}{spec[1]}-{m}" if spec else f"{what}-{m}"
