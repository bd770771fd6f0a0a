#!/usr/bin/env python3
"""Golden vectors for the JPEG 2000 base layer ALONE, generated with the real OpenJPEG 2.4.0 of this image through the
oracle's optional backend (oracle/opj_backend.c: the reference's own call sequence, /root/reference/src/ebcc_codec.c:105-180
encode and :1092-1136 decode, on a u16 image).  TEST INFRASTRUCTURE; run in the dev container only:

    python3 oracle/make_golden_j2k.py          ->  tests/golden/j2k_openjpeg.json, tests/golden/j2k_inputs.npz
    python3 oracle/make_golden_j2k.py fields   ->  tests/golden/j2k_fields.json

tests/test_oracle_golden.py::test_j2k_restatement_against_openjpeg_fixtures pins oracle/j2k_oracle.c on them on any box
(the live comparison with the library only runs where the library is).  Inputs are integer formulas (reproducible
anywhere) or stored arrays; small codestreams are stored whole, large ones as sha256.

`fields` covers the frame sizes real callers hit (1024 x 1024 chunks, the largest legal 2047 x 2047, the thinnest) with
the high-entropy content of tests/_fields.py at the whole rate ladder of tests/test_j2k_gpu.py, as hashes only: the
input frame, the codestream, the decoded samples and the samples mapped back to float32 (ebcc_codec.c:1130).  The GPU
tests compare the product with these directly; the CPU test pins the oracle on the cases marked "pin" (every rate at
the small shapes, a trimmed ladder at the two biggest)."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _lib as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def formula_u16(h, w, k=0):
    """smooth ramps + blocks + fine texture, exactly reproducible"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    v = (x * x * 3 + y * y * 5 + x * y * (k + 1)) % 4096 * 12 + ((x // 16) * 7 + (y // 16) * 13 + k) % 97 * 160 + (x * 7 + y * 13) % 31
    return np.ascontiguousarray((v % 65536).astype(np.uint16))


def main():
    lib = L.oracle()
    assert hasattr(lib, "orc_opj_encode") and L.opj_version().startswith("2.4.0"), "needs the OpenJPEG 2.4.0 backend: " + repr(L.opj_version())

    def enc(img, cr):
        out = ctypes.c_void_p()
        n = lib.orc_opj_encode(img.ctypes.data, img.shape[0], img.shape[1], ctypes.c_float(cr), ctypes.byref(out))
        s = ctypes.string_at(out.value, n)
        lib.orc_free(out)
        return s

    def dec(s):
        b = ctypes.create_string_buffer(s, len(s))
        out, h, w = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        n = lib.orc_opj_decode(b, len(s), ctypes.byref(out), ctypes.byref(h), ctypes.byref(w))
        a = np.frombuffer(ctypes.string_at(out.value, 4 * n), np.int32).copy()
        lib.orc_free(out)
        return a

    arrays, cases = {}, []
    stored = {"nat_48x80": (48, 80, 11), "nat_96x160": (96, 160, 12)}
    for name, (h, w, seed) in stored.items():
        f = L.era5_like(h, w, seed, 1.2, 1.5)
        arrays[name] = np.ascontiguousarray((((f - f.min()) / (f.max() - f.min())) * np.float32(65535)).astype(np.uint16))
    inputs = [("formula", (32, 32, 0)), ("formula", (45, 70, 1)), ("formula", (64, 96, 2)), ("formula", (100, 130, 3)), ("formula", (181, 360, 4)),
              ("formula", (721, 1440, 5)), ("stored", "nat_48x80"), ("stored", "nat_96x160")]
    for kind, spec in inputs:
        img = formula_u16(*spec) if kind == "formula" else arrays[spec]
        big = img.size > 20000
        for cr in ((30.0, 100.0) if img.size > 500000 else (1.0, 4.0, 17.0, 60.0, 900.0)):
            s = enc(img, cr)
            c = {"input": kind, "spec": spec, "h": int(img.shape[0]), "w": int(img.shape[1]), "cr": cr, "n": len(s),
                 "stream_sha256": hashlib.sha256(s).hexdigest(), "decoded_sha256": hashlib.sha256(dec(s).tobytes()).hexdigest()}
            if not big:
                c["stream_hex"] = s.hex()
            cases.append(c)
    np.savez_compressed(os.path.join(OUT, "j2k_inputs.npz"), **arrays)
    json.dump({"openjpeg": L.opj_version(), "cases": cases}, open(os.path.join(OUT, "j2k_openjpeg.json"), "w"), indent=0)
    print(len(cases), "cases,", sum(len(c.get("stream_hex", "")) // 2 for c in cases), "stream bytes stored")


FIELD_SHAPES = [(257, 383), (1024, 1024), (2047, 2047), (2047, 33), (32, 2047)]
FIELD_RATES = [1.0, 3.0, 7.5, 30.0, 120.0, 1000.0]                 # tests/test_j2k_gpu.py RATES
PIN_RATES = {(1024, 1024): (1.0, 30.0), (2047, 2047): (1.0, 1000.0)}


def _field_case(job):
    kind, h, w, cr = job
    from tests import _fields as F
    lib = L.oracle()
    x = F.field(kind, h, w)
    u16, mn, mx = L.scale_u16(x)
    out = ctypes.c_void_p()
    n = lib.orc_opj_encode(u16.ctypes.data, h, w, ctypes.c_float(cr), ctypes.byref(out))
    s = ctypes.string_at(out.value, n)
    lib.orc_free(out)
    b = ctypes.create_string_buffer(s, len(s))
    out, dh, dw = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
    m = lib.orc_opj_decode(b, len(s), ctypes.byref(out), ctypes.byref(dh), ctypes.byref(dw))
    samples = np.frombuffer(ctypes.string_at(out.value, 4 * m), np.int32).reshape(h, w).copy()
    lib.orc_free(out)
    return {"kind": kind, "h": h, "w": w, "cr": cr, "pin": cr in PIN_RATES.get((h, w), FIELD_RATES),
            "field_sha256": F.sha(x.tobytes()), "n": len(s), "stream_sha256": F.sha(s),
            "decoded_sha256": F.sha(samples.tobytes()), "mapped_sha256": F.sha(L.map_decoded(samples, mn, mx).tobytes())}


def fields():
    import multiprocessing as mp
    from tests import _fields as F
    assert hasattr(L.oracle(), "orc_opj_encode") and L.opj_version().startswith("2.4.0"), "needs the OpenJPEG 2.4.0 backend"
    jobs = [(k, h, w, cr) for h, w in FIELD_SHAPES for k in F.KINDS for cr in FIELD_RATES]
    with mp.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as pool:
        cases = pool.map(_field_case, jobs, chunksize=1)
    json.dump({"openjpeg": L.opj_version(), "cases": cases}, open(os.path.join(OUT, "j2k_fields.json"), "w"), indent=0)
    print(len(cases), "cases,", sum(c["pin"] for c in cases), "pinned on the oracle")


if __name__ == "__main__":
    fields() if sys.argv[1:] == ["fields"] else main()
