"""GPU: the rate-independent half of the JPEG 2000 encoder against the oracle, table by table and code-block by code-block.

The codestream tests (tests/test_j2k_gpu.py, the golden streams) see the forward transform, the six fractional bits of Q6, the
per-pass rates and the distortion doubles only through the bytes that survive a cut: a distortion that is off in its low bits
moves a layer decision only where a slope threshold happens to lie there.  Here ebcc_hip_j2k_tables hands out what the
analysis left in the context, and every value is compared exactly (doubles and floats by bit pattern) with the oracle's
analysis of the same u16 image (tests/_j2k_tables.py), so that a departure is reported with its stage, frame, code-block and
first pass or sample instead of as a stream hash.

The shapes are the smallest that hold 1x1 and 1xN code-blocks, code-blocks narrower than 64 with a height that is no
multiple of 4, widths of 32k + 1 at several levels, and more than 64 code-blocks a frame (the 64-block groups of the
lane-interleaved arrays are cut inside a frame and between frames)."""
import numpy as np
import pytest

from tests import _j2k_tables as T
from tests import _lib as L
from tests.test_j2k_gpu import RATES
from tests.test_probe_j2k_gpu import KEEP_MODES, WALKS

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (33, 47), (100, 130), (330, 520), (64, 2047), (2047, 33)]
# what the oracle holds for these shapes (asserted below, so that a comparison of nothing cannot pass): code-blocks a frame,
# and the code-blocks without a coding pass of the spike and the checker frame
BLOCKS = dict(zip(SHAPES, (16, 16, 19, 76, 94, 94)))
EMPTY = {"spike": dict(zip(SHAPES, (0, 0, 3, 57, 66, 78))), "checker": dict(zip(SHAPES, (14, 14, 16, 60, 77, 77)))}
MOST_PASSES = 61


def _ids(s):
    return f"{s[0]}x{s[1]}"


def _oracle_side(h, w, kinds):
    """the conditions on the oracle's tables that make the comparison mean something"""
    per_frame = BLOCKS[(h, w)]
    most, narrow = 0, 0
    for kind in set(kinds) - {"constant"}:
        want, seconds = T.oracle_blocks(kind, h, w)
        assert len(want) == per_frame, (kind, len(want))
        empty = sum(1 for b in want if b["totalpasses"] == 0)
        if kind in EMPTY:
            assert empty == EMPTY[kind][(h, w)], (kind, empty)
            assert empty < per_frame, kind                               # at least one coded code-block
        else:
            assert empty == 0, (kind, empty)
        for b in want:
            assert b["totalpasses"] == 0 or (b["len"] > 0 and len(b["rates"]) == len(b["disto"]) == b["totalpasses"] and
                                             len(b["bytes"]) == b["len"]), kind
        most = max(most, max(b["totalpasses"] for b in want))
        narrow += sum(1 for b in want if b["w"] < 64 and b["h"] % 4)
        assert seconds < T.ORACLE_SECONDS, (kind, seconds)
    return most, narrow


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_tables_bit_exact(shape):
    h, w = shape
    per_frame = BLOCKS[shape]
    most, narrow = _oracle_side(h, w, T.BATCH)
    assert most == MOST_PASSES <= L.J2K_MAX_PASSES, most
    assert (narrow > 0) == (shape != (64, 2047)), narrow
    with L.Context(len(T.BATCH), h, w) as ctx:
        t = ctx.j2k_tables(T.batch(h, w))
    assert t.nblocks == per_frame and t.retried == 0
    compared = 0
    for f, kind in enumerate(T.BATCH):
        if kind == "constant":
            T.constant_frame_is_left_out(t, f)
            continue
        assert t.const[f] == 0, f"frame {f} ({kind}) is flagged constant"
        compared += T.compare_frame(t, f, kind)
    assert compared == 5 * per_frame, compared
    assert list(t.const) == [int(k == "constant") for k in T.BATCH]
    T.same_tables(t, 0, t, 5, f"{h}x{w}: the two era5_like frames (0 and 5)")
    # the packed arrays hold nothing but the code-blocks' passes and bytes, in order
    k = t.blocks.reshape(-1)
    assert np.array_equal(k["pass_at"], np.concatenate([[0], np.cumsum(k["totalpasses"][:-1])]))
    assert np.array_equal(k["byte_at"], np.concatenate([[0], np.cumsum(k["len"][:-1])]))


def test_tables_do_not_depend_on_the_encoder_form(monkeypatch):
    """the segmented two-phase encoder, the single-kernel one, and the retry of the second after the first ran out of decision
    rows (tests/test_codec_gpu.py: test_tier1_retry_when_decisions_outgrow_their_rows) leave the same tables"""
    h, w = 100, 130
    kinds = ("noise", "checker")
    _oracle_side(h, w, kinds)
    frames = T.batch(h, w, kinds)
    got = {}
    for name, env in (("default", {}), ("single-kernel", {"EBCC_T1_TWO_PHASE": "0"}), ("retry", {"EBCC_HIP_SYM_ROWS": "40"})):
        for k in ("EBCC_T1_TWO_PHASE", "EBCC_HIP_SYM_ROWS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with L.Context(len(kinds), h, w) as ctx:
            got[name] = ctx.j2k_tables(frames)
    assert got["default"].retried == 0 and got["single-kernel"].retried == 0
    assert got["retry"].retried == 1, "the decisions did not outgrow 40 rows: the retry did not run"
    for name, t in got.items():
        for f, kind in enumerate(kinds):
            assert T.compare_frame(t, f, kind) == BLOCKS[(h, w)], name
    for name in ("single-kernel", "retry"):
        for f in range(len(kinds)):
            T.same_tables(got["default"], f, got[name], f, f"{name} against default, frame {f}")


@pytest.mark.parametrize("shape", [(33, 47), (330, 520)], ids=_ids)
def test_tables_survive_rate_allocation_and_probes(shape):
    """k_rate, its cache and the probes' restart decode read the tables and must not write them: after encodes at every rate
    of the ladder and the hostile walk of the probes, the context still holds the oracle's tables"""
    h, w = shape
    _oracle_side(h, w, T.BATCH)
    frames = T.batch(h, w)
    n = len(frames)
    live = np.array([int(k != "constant") for k in T.BATCH], np.int32)
    span = np.array([float(x.max() - x.min()) for x in frames], np.float32)
    with L.Context(n, h, w) as ctx:
        for cr in RATES:
            streams, _, d = ctx.j2k_encode(frames, [cr] * n, keep_device=True)
            assert [len(s) > 0 for s in streams] == [bool(v) for v in live], cr
            if cr != RATES[-1]:
                d.free()
        for i, cr in enumerate(WALKS["hostile"]):
            keep = [(f + i) % 2 for f in range(n)]
            nbad, _, size, _ = ctx.j2k_probe(d, n, float(cr), span * np.float32(0.01), keep=keep, active=live, keep_field=KEEP_MODES[i])
            for f in range(n):
                if live[f]:
                    assert size[f] > 0 and nbad[f] != L.Context.PROBE_SENTINEL[0], (f, cr)
        d.free()
        t = ctx.j2k_tables(None, n)
    assert t.coeffs is None and list(t.const) == list(1 - live)
    compared = 0
    for f, kind in enumerate(T.BATCH):
        if kind == "constant":
            T.constant_frame_is_left_out(t, f)
            continue
        compared += T.compare_frame(t, f, kind, [s for s in T.STAGES if s != "coefficients"])
    assert compared == 5 * BLOCKS[shape]
    T.same_tables(t, 0, t, 5, f"{h}x{w}: the two era5_like frames (0 and 5)", coeffs=False)
