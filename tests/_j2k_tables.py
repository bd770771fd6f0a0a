"""The rate-independent tables of the JPEG 2000 encoder - forward 9/7 coefficients, Q6, tier-1 with its per-pass byte
counts, the distortion sums - as ebcc_hip_j2k_tables returns them, against the oracle's analysis of the same frame
(tests/_lib.py: orc_j2k_analysis), code-block by code-block.  Every comparison is exact: integers as integers, floats and
doubles by bit pattern.  A mismatch names the stage, the shape, the frame, the code-block (band, rectangle) and the first
pass or sample that differs (tests/test_j2k_tables_gpu.py).

A chunk of several frames is one image with a tile per frame: its content is a tuple of kinds, one per tile, the oracle's
code-blocks are those of one tile position of the stacked image scaled by the chunk, and the tables come from a context
for chunks (tests/test_tile_positions_gpu.py)."""
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


# The tiles of a chunk share one (min, max).  The kinds of F.field live on [0, 1] and era5_like near 235 .. 290, so a tile of
# a chunk is brought to [CHUNK_LO, CHUNK_LO + CHUNK_SPAN] = [180, 300] (one float32 multiply and add: the same bits anywhere):
# noise and checkerboard then span the chunk's whole range next to an era5_like tile, not its lowest 1/290.
# "mid" and "unit_spike" are for a chunk of range [0, 1] whose other tiles hold nothing: mid is a constant that scales to
# u16 32768, which the level shift takes to 0, so every coefficient of such a tile is 0 and every code-block of it empty.
CHUNK_LO, CHUNK_SPAN = np.float32(180.0), np.float32(120.0)
MID = np.float32(0.50001)
assert int(MID * np.float32(65535)) == 32768


@functools.lru_cache(maxsize=None)
def tile_frame(kind, h, w):
    if kind in ("era5_like", "constant"):
        x = frame(kind, h, w)
        assert CHUNK_LO <= x.min() and x.max() <= CHUNK_LO + CHUNK_SPAN, kind
        return x
    if kind == "mid":
        return np.full((h, w), MID, np.float32)
    if kind == "unit_spike":
        return F.field("spike", h, w)
    return (CHUNK_LO + CHUNK_SPAN * F.field(kind, h, w)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def chunk(kinds, h, w):
    """[len(kinds)][h][w]: the chunk whose tile k holds tile_frame(kinds[k]) (shared, never written to)"""
    x = np.stack([tile_frame(k, h, w) for k in kinds])
    x.setflags(write=False)
    return x


def chunk_u16(kinds, h, w):
    """the stacked image of the chunk as the encoder scales it: with the chunk's (min, max)"""
    return L.scale_u16(chunk(kinds, h, w))[0]


@functools.lru_cache(maxsize=None)
def oracle_blocks(kind, h, w, tile=0):
    """the oracle's code-blocks of L.scale_u16 of the frame (computed once, shared, never written to) and the CPU seconds
    the analysis took (the least of up to three runs, the later ones made only if the first is not under ORACLE_SECONDS).
    kind a tuple: the code-blocks of tile position `tile` of that chunk."""
    u16 = chunk_u16(kind, h, w) if isinstance(kind, tuple) else L.scale_u16(frame(kind, h, w))[0]
    t0 = time.process_time()
    blocks = L.orc_j2k_analysis(u16, tile)
    seconds = time.process_time() - t0
    for _ in range(2):
        if seconds < ORACLE_SECONDS:
            break
        t0 = time.process_time()
        L.orc_j2k_analysis(u16, tile)
        seconds = min(seconds, time.process_time() - t0)
    for b in blocks:
        for k in ("q", "cf", "rates", "disto"):
            b[k].setflags(write=False)
    return tuple(blocks), seconds


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def where(t, f, b, kind, tile=0):
    k = t.blocks[f, b]
    if isinstance(kind, tuple):
        kind = f"{kind[tile]} of {'+'.join(kind)}"
    return (f"{t.h}x{t.w} frame {f} tile position {tile} ({kind}) code-block {b}: resolution {k['res']} {ORIENT[k['orient']]}, "
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


def compare_block(t, f, b, want, kind, stages=STAGES, tile=0):
    """code-block b of frame f of the tables t against the oracle's code-block `want`, stage by stage"""
    k = t.blocks[f, b]
    at = where(t, f, b, kind, tile)
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


def own_blocks(t, f, tile=0):
    """the code-blocks frame f has at its tile position: the leading slots, which hold a rectangle.  The slots behind them
    (a context for chunks has as many a frame as its largest tile position needs) hold no rectangle, passes or bytes."""
    k = t.blocks[f]
    own = int(np.count_nonzero(k["w"] * k["h"]))
    rest = k[own:]
    assert (k["w"][:own] > 0).all() and (k["h"][:own] > 0).all(), f"frame {f} tile position {tile}: a slot without a rectangle before slot {own}"
    for name in ("x", "y", "w", "h", "numbps", "totalpasses", "len"):
        assert not rest[name].any(), f"frame {f} tile position {tile}: a slot past code-block {own - 1} is not empty: {name} {rest[name].tolist()}"
    return own


def compare_frame(t, f, kind, stages=STAGES, tile=0):
    """every code-block of frame f against the oracle (kind a tuple: against tile position `tile` of that chunk); returns
    the number compared"""
    want, _ = oracle_blocks(kind, t.h, t.w, tile)
    own = own_blocks(t, f, tile)
    assert len(want) == own, f"{t.h}x{t.w} tile position {tile}: {own} code-blocks a frame against the oracle's {len(want)}"
    # stage-major: the report is the earliest stage that departs anywhere in the frame, not the first code-block's latest
    for stage in stages:
        for b in range(own):
            compare_block(t, f, b, want[b], kind, (stage,), tile)
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


# ---- chunks of several frames: a tile per frame, a geometry per tile position (tests/test_tile_positions_gpu.py; the
#      fixture tests/golden/tile_positions.json is written by oracle/make_golden_tiles.py from these)
TILE_KINDS = ("era5_like", "noise", "spike", "checker")
# (tiles, height, width): the smallest shapes that hold each effect
CHUNKS = [(2, 33, 35),      # odd height: tile 1 at odd parity on five resolutions; 1xN and 1-line code-blocks
          (3, 37, 70),      # three parity patterns
          (4, 34, 70),      # height = 2 mod 4: tile 3 has more code-blocks than tiles 0 - 2, which leave padding slots
          (5, 36, 47),      # height = 4 mod 8: five positions, tile 3 has the extra code-blocks
          (3, 63, 130),     # tile 2's level-1 bands start at 63 mod 64: a first code-block row of one line above a second
          (2, 127, 33),     # the same in a thin tile, for the high-pass bands only
          (2, 48, 2047),    # height = 16 mod 32: one resolution changes parity; 64-block groups are cut inside and between tiles
          (2, 100, 130)]    # an odd shape with hostile content
ROTATIONS = (0, 1, 2, 3)


def rotated(tiles, r):
    """the kinds of a chunk's tiles: TILE_KINDS in order from number r, so that over the four rotations every kind visits
    every tile position"""
    return tuple(TILE_KINDS[(k + r) % len(TILE_KINDS)] for k in range(tiles))


SPECIAL_SHAPES = [(3, 37, 70), (3, 63, 130)]
SPECIAL = {"constant-tile": ("noise", "constant", "checker"),          # a constant tile among live ones: it is coded
           "spike-among-constants": ("mid", "mid", "unit_spike"),      # every code-block of the other tiles is empty
           "constant-chunk": ("constant", "constant", "constant")}
# the bounded modes of the fixture: (mode, error, base_cr, quantile, rotation), with the pure-base fallback disabled so that
# the residual layer over the stacked image stays and the chunk-level search runs
BOUNDED = [(L.MAX_ERROR, 0.5, 20.0, "0.1", 0), (L.RELATIVE_ERROR, 2e-3, 20.0, "0.3", 2)]
BOUNDED_ENV = ("EBCC_INIT_BASE_ERROR_QUANTILE", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK")


def chunk_id(shape, kinds):
    return "x".join(str(v) for v in shape) + "-" + "+".join(kinds)


def fixture_chunks():
    """(shape, kinds) of every chunk of tests/golden/tile_positions.json: the catalogue under every rotation, the special chunks"""
    return [(s, rotated(s[0], r)) for s in CHUNKS for r in ROTATIONS] + [(s, kinds) for s in SPECIAL_SHAPES for kinds in SPECIAL.values()]


def bounded_modes(shape, kinds):
    """(mode, error, base_cr, quantile) of the BOUNDED cases the fixture holds for this chunk"""
    return [b[:4] for b in BOUNDED if shape in CHUNKS and kinds == rotated(shape[0], b[4])]


def rate_key(shape, kinds, cr):
    return f"{chunk_id(shape, kinds)}-none-cr{cr:g}"


def bounded_key(shape, kinds, mode):
    return chunk_id(shape, kinds) + {L.MAX_ERROR: "-abs", L.RELATIVE_ERROR: "-rel"}[mode]
