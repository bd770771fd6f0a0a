"""GPU: the whole codec at the frame sizes real callers hit, bit-exact against the reference build
(tests/golden/large_frames.json, oracle/make_golden_large.py; the CPU suite pins the oracle on a sample of it).

- 1024 x 1024 (the chunk ebcc_encode_chunking_compat picks for any dimension above 2047) and 2047 x 2047 (the largest
  legal frame): one batch per shape through Context.encode_frames / decode_frames, value domains of tests/_domains.py
  mixed with the high-entropy fields of tests/_fields.py, in MAX_ERROR and RELATIVE_ERROR;
- ebcc_encode_chunking_compat / ebcc_decode_chunking with no chunk shape on a (2, 2100, 1100) array: default 1024-row
  chunks, a 52-row edge chunk, and in RELATIVE_ERROR the bound over the whole array's range.  The reference misses
  the MAX_ERROR bound there (0.0511 against 0.05); parity with it, not the bound, is what that case asserts.
Every input is checked against the sha256 the fixture recorded, so a platform difference fails as "input differs"."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import _fields as F
from tests import _lib as L

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(L.GOLDEN, "large_frames.json")))
CASES = FIXTURE["cases"]
MODE_IDS = {L.MAX_ERROR: "abs", L.RELATIVE_ERROR: "rel"}


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(autouse=True)
def _default_search(monkeypatch):
    monkeypatch.delenv("EBCC_INIT_BASE_ERROR_QUANTILE", raising=False)


@pytest.mark.parametrize("mode,err", F.LARGE_MODES, ids=[MODE_IDS[m] for m, _ in F.LARGE_MODES])
@pytest.mark.parametrize("batch", sorted(F.LARGE_BATCHES))
def test_batch_streams_and_fields(batch, mode, err):
    (h, w), specs = F.LARGE_BATCHES[batch]
    frames = np.stack([F.large_frame(k, h, w, seed) for k, seed in specs])
    want = [CASES[F.large_key(batch, spec, mode)] for spec in specs]
    for spec, x, c in zip(specs, frames, want):
        assert sha(x.tobytes()) == c["field_sha256"], f"input differs: {spec}"
    cfg = L.make_config((1, h, w), base_cr=FIXTURE["base_cr"], error=err, residual_type=mode)
    with L.Context(len(frames), h, w) as ctx:
        got = ctx.encode_frames(frames, cfg)
        dec = ctx.decode_frames(got)
    for f, (spec, c) in enumerate(zip(specs, want)):
        assert len(got[f]) == c["n"] and sha(got[f]) == c["stream_sha256"], spec
        assert sha(dec[f].tobytes()) == c["decoded_sha256"], spec
        tgt = err if mode == L.MAX_ERROR else err * (float(frames[f].max()) - float(frames[f].min()))
        assert np.abs(dec[f].astype(np.float64) - frames[f]).max() <= tgt * 1.01 + 1e-4, spec


@pytest.mark.parametrize("mode,err", F.LARGE_MODES, ids=[MODE_IDS[m] for m, _ in F.LARGE_MODES])
def test_chunking_compat_default_chunks(mode, err):
    lib = L.product()
    x = F.compat_array()
    c = CASES[F.large_key("compat", None, mode)]
    assert sha(x.tobytes()) == c["field_sha256"], "input differs"
    cfg = L.make_config(F.COMPAT_SHAPE, base_cr=FIXTURE["base_cr"], error=err, residual_type=mode)
    out = ctypes.c_void_p()
    n = lib.ebcc_encode_chunking_compat(x.ctypes.data, ctypes.byref(cfg), ctypes.byref(out))
    assert n > 0 and out
    s = ctypes.string_at(out.value, n)
    lib.free_buffer(out)
    assert len(s) == c["n"] and sha(s) == c["stream_sha256"]
    b = ctypes.create_string_buffer(s, len(s))
    out = ctypes.c_void_p()
    m = lib.ebcc_decode_chunking(b, len(s), ctypes.byref(out))
    assert m == x.size and out
    dec = np.frombuffer(ctypes.string_at(out.value, 4 * m), np.float32).copy()
    lib.free_buffer(out)
    assert sha(dec.tobytes()) == c["decoded_sha256"]
    # (no bound check: in MAX_ERROR the reference's own container misses 0.05 on this array by about 2%, 0.0511, and the
    # product reproduces it bit for bit)
