#!/usr/bin/env python3
"""Golden hashes for the whole codec at the frame sizes real callers hit, written by the reference build
(oracle/_ref/libh5z_ebcc_ref.so).  TEST INFRASTRUCTURE; run in the dev container only:

    python3 oracle/make_golden_large.py      ->  tests/golden/large_frames.json

Hashes only (input frame, stream, decoded field), so the fixture stays small:
- batch_1024 / batch_2047: one frame per ebcc_encode (dims (1, h, w)), value domains of tests/_domains.py mixed with
  the high-entropy fields of tests/_fields.py, in MAX_ERROR and RELATIVE_ERROR.  1024 x 1024 is the chunk
  ebcc_encode_chunking_compat picks for any dimension above 2047; 2047 x 2047 is the largest legal frame.
- extreme: the 2047 x 2047 frame of tests/test_codec_gpu.py::test_extreme_frame_sizes.
- compat: ebcc_encode_chunking_compat with no chunk shape on a (2, 2100, 1100) array: default 1024-row chunks with a
  52-row edge chunk, and in RELATIVE_ERROR the bound taken over the whole array's range (src/ebcc_codec.c:1054-1090).
- spiht: the residual coder alone (oracle/_ref/libspiht_ref.so) on the noise, spike and checkerboard images of
  tests/test_residual_gpu.py at its large shapes, untruncated (a buffer of h*w*4 bytes, src/spiht/spiht_re.c:433) and
  truncated.

tests/test_oracle_golden.py pins the oracle on a sample of these (the restated search takes tens of seconds per
full-size frame) and re-runs that sample on the reference build where it is present; tests/test_large_frames_gpu.py
compares the product with every case."""
import ctypes
import hashlib
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _fields as F  # noqa: E402
from tests import _lib as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "large_frames.json")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _ref():
    lib = L.reference()
    for name in ("ebcc_encode_chunking_compat",):
        f = getattr(lib, name)
        f.restype = ctypes.c_size_t
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(L.CodecConfig), L.c_void_pp]
    lib.ebcc_decode_chunking.restype = ctypes.c_size_t
    lib.ebcc_decode_chunking.argtypes = [ctypes.c_void_p, ctypes.c_size_t, L.c_void_pp]
    return lib


def _run(lib, x, cfg, enc, dec):
    out = ctypes.c_void_p()
    n = getattr(lib, enc)(x.ctypes.data, ctypes.byref(cfg), ctypes.byref(out))
    assert n > 0, "the reference wrote no stream"
    s = ctypes.string_at(out.value, n)
    lib.free_buffer(out)
    b = ctypes.create_string_buffer(s, len(s))
    out = ctypes.c_void_p()
    m = getattr(lib, dec)(b, len(s), ctypes.byref(out))
    d = ctypes.string_at(out.value, 4 * m)
    lib.free_buffer(out)
    return {"field_sha256": sha(x.tobytes()), "n": len(s), "stream_sha256": sha(s), "decoded_sha256": sha(d)}


def _job(job):
    os.environ.pop("EBCC_INIT_BASE_ERROR_QUANTILE", None)
    lib = _ref()
    what, spec, mode, err = job
    if what == "compat":
        x = F.compat_array()
        cfg = L.make_config(F.COMPAT_SHAPE, base_cr=F.LARGE_BASE_CR, error=err, residual_type=mode)
        return _run(lib, x, cfg, "ebcc_encode_chunking_compat", "ebcc_decode_chunking")
    if what == "extreme":
        x = F.extreme_frame()
        cfg = L.make_config((1, 2047, 2047), base_cr=40.0, error=err, residual_type=mode)
    else:
        (h, w), (kind, seed) = F.LARGE_BATCHES[what][0], spec
        x = F.large_frame(kind, h, w, seed)
        cfg = L.make_config((1, h, w), base_cr=F.LARGE_BASE_CR, error=err, residual_type=mode)
    return _run(lib, x, cfg, "ebcc_encode", "ebcc_decode")


SPIHT_SHAPES = [(1024, 1024), (2047, 2047), (2047, 33)]
SPIHT_IMAGES = [("noise", 7), ("spike", 0), ("checker", 0)]


def spiht_trunc_bits(h, w):
    return [0, 1024, 8 * (h * w // 20)]                   # tests/test_residual_gpu.py::test_streams_bit_exact


def _spiht_job(job):
    (h, w), (kind, seed), tb = job
    sp = ctypes.CDLL(L.REF_SPIHT_SO)
    sp.spiht_encode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, L.c_void_pp, L.c_size_p,
                                ctypes.c_size_t, ctypes.c_size_t]
    sp.spiht_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                ctypes.c_size_t]
    x = F.field(kind, h, w, seed)
    buf, n = ctypes.c_void_p(), ctypes.c_size_t()
    sp.spiht_encode(x.ctypes.data, h, w, ctypes.byref(buf), ctypes.byref(n), tb, 3)
    s = ctypes.string_at(buf.value, n.value)
    out = np.zeros((h, w), np.float32)
    sp.spiht_decode(buf.value, n.value, out.ctypes.data, h, w, 8 * n.value)
    return {"kind": kind, "seed": seed, "h": h, "w": w, "trunc_bits": tb, "field_sha256": sha(x.tobytes()), "n": len(s),
            "stream_sha256": sha(s), "decoded_sha256": sha(out.tobytes())}


def jobs():
    out = []
    for what, (_, frames) in F.LARGE_BATCHES.items():
        out += [(what, spec, mode, err) for mode, err in F.LARGE_MODES for spec in frames]
    out += [("extreme", None, mode, err) for mode, err in F.EXTREME_MODES]
    out += [("compat", None, mode, err) for mode, err in F.LARGE_MODES]
    # the longest first: the 2047 x 2047 noise frames and the compat arrays
    return sorted(out, key=lambda j: (j[0] not in ("batch_2047", "extreme", "compat"), j[1] != ("noise", 1)))


def main():
    assert L.reference() is not None, "needs the reference build (oracle/_ref)"
    todo = jobs()
    with mp.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_job, todo, chunksize=1)
        spiht = pool.map(_spiht_job, [(s, im, tb) for s in SPIHT_SHAPES for im in SPIHT_IMAGES for tb in spiht_trunc_bits(*s)])
    cases = {F.large_key(w, s, m): dict(r, error=e, mode=m) for (w, s, m, e), r in zip(todo, res)}
    json.dump({"base_cr": F.LARGE_BASE_CR, "cases": dict(sorted(cases.items())), "spiht": spiht}, open(OUT, "w"), indent=0)
    print(len(cases), "cases,", len(spiht), "residual streams")


if __name__ == "__main__":
    main()
