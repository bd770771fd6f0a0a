"""GPU parity of the JPEG 2000 base layer against the CPU oracle (itself pinned to OpenJPEG 2.4.0):
codestreams bit-exact, decoded fields bit-exact (the contract allows 1 ULP; we get 0).

The smooth fields run at SHAPES against the live oracle.  The high-entropy fields of tests/_fields.py run at
FIELD_SHAPES (1024 x 1024 chunks, the largest legal frame, the thinnest) against what OpenJPEG 2.4.0 wrote for them
(tests/golden/j2k_fields.json, oracle/make_golden_j2k.py; the CPU suite pins the oracle on the same cases): one frame at
every rate of the ladder per test, parametrize ids "<h>x<w>-<field>"."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import _fields as F
from tests import _lib as L

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (33, 47), (64, 96), (100, 130), (181, 360), (721, 1440)]
RATES = [1.0, 3.0, 7.5, 30.0, 120.0, 1000.0]
FIELD_SHAPES = [(257, 383), (1024, 1024), (2047, 2047), (2047, 33), (32, 2047)]
FIXTURE = {(c["kind"], c["h"], c["w"], c["cr"]): c
           for c in json.load(open(os.path.join(L.GOLDEN, "j2k_fields.json")))["cases"]}
FIELD_CASES = [pytest.param((h, w, k), id=f"{h}x{w}-{k}") for h, w in FIELD_SHAPES for k in F.KINDS]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _field_batch(h, w, kind):
    """the field once per rate of the ladder, and the fixture of each"""
    x = F.field(kind, h, w)
    want = [FIXTURE[(kind, h, w, cr)] for cr in RATES]
    assert sha(x.tobytes()) == want[0]["field_sha256"], f"input differs: {kind} {h}x{w}"
    return x, np.stack([x] * len(RATES)), want


def _field_streams(ctx, h, w, kind):
    """the product's codestreams of one field at every rate, checked against OpenJPEG's (hashes)"""
    x, frames, want = _field_batch(h, w, kind)
    got, mm = ctx.j2k_encode(frames, RATES)
    _, mn, mx = L.scale_u16(x)
    for i, cr in enumerate(RATES):
        assert mm[i, 0] == mn and mm[i, 1] == mx, cr
        assert len(got[i]) == want[i]["n"] and sha(got[i]) == want[i]["stream_sha256"], (kind, cr)
    return x, got, (mn, mx), want


def _field_codestreams(h, w, kind, monkeypatch):
    monkeypatch.delenv("EBCC_T1_TWO_PHASE", raising=False)
    with L.Context(len(RATES), h, w) as ctx:
        x, got, _, _ = _field_streams(ctx, h, w, kind)
    if kind in ("noise", "checker"):
        # the single-kernel encoder (also the retry after a group's decisions outgrow their rows of SYM) writes the same
        # codestreams as the segmented one at its decision budget, whether or not that overflowed
        monkeypatch.setenv("EBCC_T1_TWO_PHASE", "0")
        with L.Context(2, h, w) as ctx:
            single, _ = ctx.j2k_encode(np.stack([x, x]), [1.0, 3.0])
        assert single == got[:2], kind


def _fields(h, w):
    return np.stack([L.era5_like(h, w, h + w), L.era5_like(h, w, h * w + 1, 1.0, 0.7),
                     (L.kat_image(h, w) * 40 + 260).astype(np.float32)])


@pytest.mark.parametrize("shape", SHAPES + FIELD_CASES)
def test_codestreams_bit_exact(shape, monkeypatch):
    if len(shape) == 3:
        return _field_codestreams(*shape, monkeypatch)
    h, w = shape
    fields = _fields(h, w)
    with L.Context(len(fields), h, w) as ctx:
        for cr in RATES:
            got, mm = ctx.j2k_encode(fields, [cr] * len(fields))
            for f, fld in enumerate(fields):
                u16, mn, mx = L.scale_u16(fld)
                assert mm[f, 0] == mn and mm[f, 1] == mx
                ref = L.orc_j2k_encode(u16, cr)
                assert len(got[f]) == len(ref), (cr, f)
                assert got[f] == ref, (cr, f)


def _field_emulated_decode(h, w, kind):
    x, frames, want = _field_batch(h, w, kind)
    target = [0.5 / 65535, 0.01, 0.05, 0.1, 0.3, 1.0]
    with L.Context(len(RATES), h, w) as ctx:
        streams, mm, d = ctx.j2k_encode(frames, RATES, keep_device=True)
        emu, nbad, esum = ctx.j2k_emulated_decode(d, len(RATES), target)
        d.free()
    for i, cr in enumerate(RATES):
        assert sha(streams[i]) == want[i]["stream_sha256"], cr
        assert sha(emu[i].tobytes()) == want[i]["mapped_sha256"], cr           # OpenJPEG's decode, mapped to float
        err = x - emu[i]
        assert int(nbad[i]) == int((np.abs(err) > np.float32(target[i])).sum()), cr
        assert abs(esum[i] - err.astype(np.float64).sum()) <= 1e-6 * max(1.0, abs(esum[i])), cr


@pytest.mark.parametrize("shape", SHAPES + FIELD_CASES)
def test_emulated_decode_equals_real_decode(shape):
    if len(shape) == 3:
        return _field_emulated_decode(*shape)
    h, w = shape
    fields = _fields(h, w)
    with L.Context(len(fields), h, w) as ctx:
        for cr in (2.0, 9.0, 40.0, 300.0):
            streams, mm, d = ctx.j2k_encode(fields, [cr] * len(fields), keep_device=True)
            target = [0.05, 0.3, 1.0]
            emu, nbad, esum = ctx.j2k_emulated_decode(d, len(fields), target)
            d.free()
            for f, fld in enumerate(fields):
                ref = L.map_decoded(L.orc_j2k_decode(streams[f]), mm[f, 0], mm[f, 1])
                assert np.array_equal(emu[f], ref), (cr, f)
                err = fld - ref
                assert int(nbad[f]) == int((np.abs(err) > np.float32(target[f])).sum())
                assert abs(esum[f] - err.astype(np.float64).sum()) <= 1e-6 * max(1.0, abs(esum[f]))


def _field_true_decode(h, w, kind):
    """every rate of the ladder, cr 1.0 (every pass kept) included"""
    with L.Context(len(RATES), h, w) as ctx:
        _, streams, mm, want = _field_streams(ctx, h, w, kind)
        got = ctx.j2k_decode(streams, [mm] * len(RATES))
    for i, cr in enumerate(RATES):
        assert sha(got[i].tobytes()) == want[i]["mapped_sha256"], (kind, cr)


@pytest.mark.parametrize("shape", SHAPES + FIELD_CASES)
def test_true_decode_bit_exact(shape):
    if len(shape) == 3:
        return _field_true_decode(*shape)
    h, w = shape
    fields = _fields(h, w)
    streams, mms = [], []
    for i, fld in enumerate(fields):
        u16, mn, mx = L.scale_u16(fld)
        streams.append(L.orc_j2k_encode(u16, [1.5, 12.0, 90.0][i]))
        mms.append((mn, mx))
    with L.Context(len(fields), h, w) as ctx:
        got = ctx.j2k_decode(streams, mms)
    for f in range(len(fields)):
        ref = L.map_decoded(L.orc_j2k_decode(streams[f]), *mms[f])
        assert np.array_equal(got[f], ref), f


DECODE_PLANS = [pytest.param({}, id="planned"), pytest.param({"EBCC_T1_LPW": "1"}, id="lpw1"),
                pytest.param({"EBCC_T1_LPW": "2"}, id="lpw2"), pytest.param({"EBCC_T1_LPW": "4"}, id="lpw4"),
                pytest.param({"EBCC_T1_DEC_TIERS": "64,8,2,8"}, id="tiers-64-8-2-8"),
                pytest.param({"EBCC_T1_DEC_TIERS": "16,4,0,16"}, id="tiers-16-4-0-16")]


@pytest.mark.parametrize("plan", DECODE_PLANS)
def test_mixed_decode_batch_under_every_lane_plan(plan, monkeypatch):
    """One 1024 x 1024 batch of spike (almost every code-block empty), smooth and full-range noise streams at every rate:
    more than 4096 code-blocks, so the decoder plans lanes and rank tiers rather than a wave per code-block.  Every plan
    decodes what OpenJPEG decodes."""
    h, w = 1024, 1024
    for k in ("EBCC_T1_LPW", "EBCC_T1_DEC_TIERS"):
        monkeypatch.delenv(k, raising=False)
    kinds = ("spike", "smooth", "noise")
    with L.Context(len(RATES) * len(kinds), h, w) as ctx:
        streams, mms, want = [], [], []
        for kind in kinds:
            _, s, mm, c = _field_streams(ctx, h, w, kind)
            streams += s
            mms += [mm] * len(s)
            want += c
        for k, v in plan.items():
            monkeypatch.setenv(k, v)
        got = ctx.j2k_decode(streams, mms)
    for i, c in enumerate(want):
        assert sha(got[i].tobytes()) == c["mapped_sha256"], (c["kind"], c["cr"])
