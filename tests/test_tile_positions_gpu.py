"""GPU: the base layer at tile positions away from the image's origin.

A chunk of F frames is one JPEG 2000 image with a tile per frame (DESIGN A.5).  A tile whose first row is not row 0 has its
own sub-band extents, its own low / high parity per resolution and its own code-block partition, anchored at absolute
multiples of 64: a first row of code-blocks of 1 to 63 lines, and another number of code-blocks than the tile at the
origin.  The engine keeps F geometries side by side (frame f uses number f % F) and a common stride of code-block slots.

The stage-level suites (tests/test_j2k_tables_gpu.py and its neighbours) run on plain frames, and the whole-codec hashes of
tests/golden/tiled.json see a tile position only through the bytes that survive one or two cuts of smooth content.  Here
- ebcc_hip_j2k_tables on a context of ebcc_hip_create_tiles hands out every tile's tables, compared exactly - integers as
  integers, floats and doubles by bit pattern - with the oracle's analysis of that tile position (tests/_j2k_tables.py),
- ebcc_encode / ebcc_decode run every chunk over the rate ladder and in both bounded modes against the oracle and against
  hashes of the reference build (tests/golden/tile_positions.json, oracle/make_golden_tiles.py; the CPU suite pins the oracle
  on the same cases),
with full-range noise, a spike, a checkerboard and a smooth field rotated through every tile position, a constant tile
among live ones, tiles whose code-blocks are all empty, and a constant chunk (tests/_j2k_tables.py: CHUNKS, SPECIAL)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from tests import _j2k_tables as T
from tests import _lib as L
from tests.test_codec_gpu import api_decode, api_encode
from tests.test_j2k_gpu import DECODE_PLANS, RATES

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(L.GOLDEN, "tile_positions.json")))["cases"]

# What the oracle holds for the catalogue (asserted below, so that a comparison of nothing cannot pass): the code-blocks of
# every tile position, and of those the ones without a coding pass where the tile is the spike or the checkerboard (every
# code-block of an era5_like or a noise tile is coded).
BLOCKS = dict(zip(T.CHUNKS, ((16, 16), (16, 16, 16), (16, 16, 16, 19), (16, 16, 16, 19, 16), (19, 19, 25), (16, 18), (94, 94), (19, 25))))
EMPTY = {"spike": dict(zip(T.CHUNKS, ((0, 0), (0, 0, 0), (0, 0, 0, 3), (0, 0, 0, 3, 0), (3, 3, 9), (0, 2), (66, 66), (3, 9)))),
         "checker": dict(zip(T.CHUNKS, ((14, 14), (14, 14, 14), (14, 14, 14, 16), (14, 14, 14, 16, 14), (16, 16, 20), (14, 15), (77, 77),
                                        (16, 20))))}
# (code-blocks, empty ones) of the tile positions of the special chunks with a tile to compare
SPECIAL_COUNTS = {((3, 37, 70), "constant-tile"): ((16, 0), (16, 15), (16, 14)),
                  ((3, 37, 70), "spike-among-constants"): ((16, 16), (16, 16), (16, 0)),
                  ((3, 63, 130), "constant-tile"): ((19, 0), (19, 18), (25, 20)),
                  ((3, 63, 130), "spike-among-constants"): ((19, 19), (19, 19), (25, 9))}
MOST_PASSES = 61
SPECIALS = [(s, name) for s in T.SPECIAL_SHAPES for name in T.SPECIAL]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _shape_id(s):
    return "x".join(str(v) for v in s)


def _param_id(v):
    """a shape, the kinds of a chunk's tiles, or a bounded mode of T.BOUNDED"""
    if isinstance(v[0], str):
        return "+".join(v)
    return _shape_id(v) if len(v) == 3 else {L.MAX_ERROR: "abs", L.RELATIVE_ERROR: "rel"}[v[0]]


def _oracle_side(shape, kinds, counts=None):
    """the conditions on the oracle's tables of the chunk that make the comparison mean something; the code-blocks of its
    tile positions"""
    f, h, w = shape
    per_tile, odd_height, most = [], 0, 0
    for k in range(f):
        want, seconds = T.oracle_blocks(kinds, h, w, k)
        assert seconds < T.ORACLE_SECONDS, (kinds, k, seconds)
        empty = sum(1 for b in want if b["totalpasses"] == 0)
        if counts is not None:
            assert (len(want), empty) == counts[k], (kinds, k, len(want), empty)
        else:
            assert len(want) == BLOCKS[shape][k], (kinds, k, len(want))
            assert empty == (EMPTY[kinds[k]][shape][k] if kinds[k] in EMPTY else 0), (kinds, k, empty)
            assert empty < len(want), (kinds, k)                         # at least one coded code-block in every tile
        for b in want:
            assert b["totalpasses"] == 0 or (b["len"] > 0 and len(b["rates"]) == len(b["disto"]) == b["totalpasses"] and
                                             len(b["bytes"]) == b["len"]), (kinds, k)
        most = max(most, max(b["totalpasses"] for b in want))
        if k > 0:                                                        # a coded code-block of one line, or of a height that is no multiple of 4
            odd_height += sum(1 for b in want if b["totalpasses"] and b["h"] % 4)
        per_tile.append(len(want))
    assert most <= L.J2K_MAX_PASSES, most
    first = [(len(T.oracle_blocks(kinds, h, w, k)[0]),) + tuple(T.oracle_blocks(kinds, h, w, k)[0][0][n] for n in ("w", "h")) for k in range(f)]
    assert any(v != first[0] for v in first[1:]), f"{shape}: every tile position has the geometry of the first: {first}"
    return per_tile, odd_height, most


def _tables(shape, chunks):
    """ebcc_hip_j2k_tables of these chunks (tuples of kinds) of one shape, side by side in one context for chunks"""
    f, h, w = shape
    frames = np.concatenate([T.chunk(kinds, h, w) for kinds in chunks])
    with L.Context(len(frames), h, w, tiles=f) as ctx:
        return ctx.j2k_tables(frames)


def _running_sums(t):
    k = t.blocks.reshape(-1)
    assert np.array_equal(k["pass_at"], np.concatenate([[0], np.cumsum(k["totalpasses"][:-1])]))
    assert np.array_equal(k["byte_at"], np.concatenate([[0], np.cumsum(k["len"][:-1])]))


def _compare_chunks(t, shape, chunks, stages=T.STAGES):
    f = shape[0]
    compared = 0
    for c, kinds in enumerate(chunks):
        for k in range(f):
            assert t.const[c * f + k] == 0, f"frame {c * f + k} is flagged constant"
            compared += T.compare_frame(t, c * f + k, kinds, stages, tile=k)
    return compared


@pytest.mark.parametrize("r", T.ROTATIONS, ids=lambda r: f"rot{r}")
@pytest.mark.parametrize("shape", T.CHUNKS, ids=_shape_id)
def test_tables_bit_exact_per_tile_position(shape, r):
    """two chunks in one context - this rotation of the kinds and the one two further, so that frame f is tile f % F of chunk
    f / F with its chunk's scaling - against the oracle's analysis of every tile at its position"""
    f, h, w = shape
    chunks = (T.rotated(f, r), T.rotated(f, (r + 2) % 4))
    per_tile, most = None, 0
    for kinds in chunks:
        per_tile, odd_height, m = _oracle_side(shape, kinds)
        assert odd_height > 0, (shape, kinds)
        most = max(most, m)
    assert set(chunks[0]) | set(chunks[1]) == set(T.TILE_KINDS) and most == MOST_PASSES, most
    t = _tables(shape, chunks)
    assert t.nblocks == max(BLOCKS[shape]) and t.retried == 0
    assert _compare_chunks(t, shape, chunks) == 2 * sum(per_tile) == 2 * sum(BLOCKS[shape])
    for c in range(2):
        for k in range(f):                                               # (compare_frame asserted the slots behind them empty)
            assert T.own_blocks(t, c * f + k, k) == BLOCKS[shape][k]
    _running_sums(t)


@pytest.mark.parametrize("shape,name", SPECIALS, ids=lambda v: _shape_id(v) if isinstance(v, tuple) else v)
def test_tables_of_constant_and_empty_tiles(shape, name):
    """a constant tile inside a live chunk is coded with the chunk's scaling; beside a spike on [0, 1] a tile at the level the
    level shift takes to 0 leaves every code-block empty; a constant chunk is left out as a whole"""
    f, h, w = shape
    kinds = T.SPECIAL[name]
    if name == "constant-chunk":
        t = _tables(shape, (kinds,))
        for k in range(f):
            T.constant_frame_is_left_out(t, k)
        return
    counts = SPECIAL_COUNTS[(shape, name)]
    _oracle_side(shape, kinds, counts)
    # beside a catalogue chunk, so that the special chunk's scaling and flags are its own
    chunks = (T.rotated(f, 1), kinds)
    t = _tables(shape, chunks)
    assert t.retried == 0
    assert _compare_chunks(t, shape, chunks) == sum(BLOCKS[shape]) + sum(c[0] for c in counts)
    for k in range(f):
        got = t.blocks[f + k][:counts[k][0]]
        assert int(np.count_nonzero(got["totalpasses"] == 0)) == counts[k][1], (k, got["totalpasses"].tolist())
    _running_sums(t)


def test_tables_do_not_depend_on_the_encoder_form(monkeypatch):
    """the segmented two-phase encoder, the single-kernel one, and the retry of the second after the first ran out of decision
    rows leave the same tables at every tile position, and those are the oracle's"""
    shape = (3, 63, 130)
    chunks = (T.rotated(3, 1), T.rotated(3, 3))
    for kinds in chunks:
        _oracle_side(shape, kinds)
    got = {}
    for name, env in (("default", {}), ("single-kernel", {"EBCC_T1_TWO_PHASE": "0"}), ("retry", {"EBCC_HIP_SYM_ROWS": "40"})):
        for k in ("EBCC_T1_TWO_PHASE", "EBCC_HIP_SYM_ROWS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got[name] = _tables(shape, chunks)
    assert got["default"].retried == 0 and got["single-kernel"].retried == 0
    assert got["retry"].retried == 1, "the decisions did not outgrow 40 rows: the retry did not run"
    for name, t in got.items():
        assert _compare_chunks(t, shape, chunks) == 2 * sum(BLOCKS[shape]), name
    for name in ("single-kernel", "retry"):
        for f in range(6):
            T.same_tables(got["default"], f, got[name], f, f"{name} against default, frame {f}")


# ---- whole chunks through ebcc_encode / ebcc_decode
@functools.lru_cache(maxsize=None)
def _oracle_ladder(shape, kinds):
    """(stream, decoded field) of the oracle in mode NONE at every rate of RATES (computed once, shared)"""
    x = T.chunk(kinds, *shape[1:])
    L.oracle().orc_set_j2k_backend(0)
    out = []
    for cr in RATES:
        s = L.orc_encode(x, L.make_config(shape, base_cr=cr, error=0.0, residual_type=L.NONE))
        assert s
        d = L.orc_decode(s)
        d.setflags(write=False)
        out.append((s, d))
    return tuple(out)


def _clear(monkeypatch):
    for k in T.BOUNDED_ENV + ("EBCC_T1_LPW", "EBCC_T1_DEC_TIERS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("shape,kinds", T.fixture_chunks(), ids=_param_id)
def test_chunk_streams_over_the_rate_ladder(shape, kinds, monkeypatch):
    """mode NONE at every rate: k_rate with its share of the main header, the packet writer over the padding slots and the
    tile-part assembly; the stream is the oracle's and the reference build's, and so is the decoded field"""
    _clear(monkeypatch)
    x = T.chunk(kinds, *shape[1:])
    for cr, (want, field) in zip(RATES, _oracle_ladder(shape, kinds)):
        c = FIXTURE[T.rate_key(shape, kinds, cr)]
        assert (len(want), sha(want), sha(field.tobytes())) == (c["n"], c["stream_sha256"], c["decoded_sha256"]), cr
        got = api_encode(x, L.make_config(shape, base_cr=cr, error=0.0, residual_type=L.NONE))
        assert len(got) == len(want) and got == want, cr
        dec = api_decode(got)
        assert T.first_difference(dec, field) is None, (cr, T.first_difference(dec, field))
        assert sha(dec.tobytes()) == c["decoded_sha256"], cr


@pytest.mark.parametrize("plan", DECODE_PLANS)
@pytest.mark.parametrize("shape", [(2, 48, 2047), (3, 63, 130)], ids=_shape_id)
def test_chunk_decode_under_every_lane_plan(shape, plan, monkeypatch):
    """every plan of the tier-1 decoder's lanes gives the oracle's field at every tile position (a chunk alone holds fewer
    code-blocks than the decoder plans rank tiers for: the two tier plans run as the planned one does, a wave per code-block;
    the three lane counts are plans of their own)"""
    _clear(monkeypatch)
    for k, v in plan.items():
        monkeypatch.setenv(k, v)
    for r in T.ROTATIONS:
        kinds = T.rotated(shape[0], r)
        for cr, (s, field) in zip(RATES, _oracle_ladder(shape, kinds)):
            d = T.first_difference(api_decode(s), field)
            assert d is None, (kinds, cr, d)


_BOUNDED = [(s, k, b) for s, k in T.fixture_chunks() for b in T.bounded_modes(s, k)]


@pytest.mark.parametrize("shape,kinds,bounded", _BOUNDED, ids=_param_id)
def test_bounded_chunks_keep_the_residual_layer(shape, kinds, bounded, monkeypatch):
    """MAX_ERROR and RELATIVE_ERROR with a quantile and without the pure-base fallback: the chunk-level rate search (summed
    counts, the header's share of every tile) and the residual layer over the stacked image; bytes and field of the
    reference build"""
    mode, err, base_cr, quantile = bounded
    _clear(monkeypatch)
    monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", quantile)
    monkeypatch.setenv("EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "1")
    c = FIXTURE[T.bounded_key(shape, kinds, mode)]
    got = api_encode(T.chunk(kinds, *shape[1:]), L.make_config(shape, base_cr=base_cr, error=err, residual_type=mode))
    assert int.from_bytes(got[16:24], "little") == c["coeffs_size"] > 0          # the residual branch is taken
    assert len(got) == c["n"] and sha(got) == c["stream_sha256"]
    assert sha(api_decode(got).tobytes()) == c["decoded_sha256"]


def test_tile_engines_of_one_frame_size_do_not_mix(monkeypatch):
    """37 x 70 frames as a chunk of three, of two, as a plain frame and as a chunk of three again, in one process: the engines
    of one frame size and different periods keep their own geometries, and the last stream is the first"""
    _clear(monkeypatch)
    x = T.chunk(T.rotated(3, 1), 37, 70)
    L.oracle().orc_set_j2k_backend(0)
    streams = []
    for tiles in (3, 2, 1, 3):
        part = np.ascontiguousarray(x[:tiles])
        for mode, cr, err in ((L.NONE, 7.5, 0.0), (L.MAX_ERROR, 20.0, 0.5)):
            cfg = L.make_config(part.shape, base_cr=cr, error=err, residual_type=mode)
            want = L.orc_encode(part, cfg)
            got = api_encode(part, cfg)
            assert want and got == want, (tiles, mode)
            d = T.first_difference(api_decode(got), L.orc_decode(want))
            assert d is None, (tiles, mode, d)
            streams.append(got)
    assert streams[6:] == streams[:2]
    assert len({s for s in streams[:6]}) == 6


def test_contexts_for_chunks_refuse_what_the_chunk_path_refuses():
    """tiles of fewer than 32 rows, an image of more than 2047 rows, no tiles at all; and tables of part of a chunk"""
    import ctypes
    lib = L.product()
    lib.ebcc_hip_create_tiles.restype = ctypes.c_void_p
    lib.ebcc_hip_create_tiles.argtypes = [ctypes.c_int] + [ctypes.c_size_t] * 4
    for frames, h, w, tiles in ((4, 31, 64, 2), (2, 1024, 64, 2), (2, 64, 64, 0), (2, 64, 2048, 2)):
        assert lib.ebcc_hip_create_tiles(0, frames, h, w, tiles) is None, (frames, h, w, tiles)
        assert lib.ebcc_hip_last_error()
    x = T.chunk(T.rotated(3, 0), 37, 70)
    with L.Context(6, 37, 70, tiles=3) as ctx:
        with pytest.raises(AssertionError, match="whole chunks"):
            ctx.j2k_tables(x[:2])
        t = ctx.j2k_tables(x)                                            # (and the context is still good)
    assert _compare_chunks(t, (3, 37, 70), (T.rotated(3, 0),)) == sum(BLOCKS[(3, 37, 70)])
    with L.Context(1, 37, 70, tiles=1) as ctx:                           # one tile: a plain context
        t = ctx.j2k_tables(T.batch(37, 70, ("noise",)))
    assert T.compare_frame(t, 0, "noise") == 16
