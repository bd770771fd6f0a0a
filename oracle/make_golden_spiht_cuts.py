#!/usr/bin/env python3
"""Golden digests of the residual coder at every bit budget and every cut of its stream, written by the reference build
(oracle/_ref/libspiht_ref.so).  TEST INFRASTRUCTURE; run in the dev container only:

    python3 oracle/make_golden_spiht_cuts.py      ->  tests/golden/spiht_cuts.json

The cases, cuts and budgets are those of tests/_spiht_cuts.py.  Per case: sha256 of the input, length and sha256 of the
stream at STREAM_BITS, and
- decode: one sha256 per WINDOW consecutive (num_bits, size) pairs of decode_pairs, over the decoded images of
  spiht_decode(stream[:size], size, ..., num_bits) one after the other;
- encode: one sha256 per WINDOW consecutive budgets of encode_budgets, over (length as 8 bytes little-endian, stream) of
  spiht_encode(image, trunc_bits) one after the other.
A mismatch then names a window of cuts or budgets.  Digests only, so the fixture stays small.

tests/test_spiht_cuts.py holds the oracle to every digest; tests/test_spiht_cuts_gpu.py compares the product with the oracle."""
import ctypes
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _lib as L  # noqa: E402
from tests import _spiht_cuts as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spiht_cuts.json")


def _ref():
    sp = ctypes.CDLL(L.REF_SPIHT_SO)
    sp.spiht_encode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, L.c_void_pp, L.c_size_p, ctypes.c_size_t,
                                ctypes.c_size_t]
    sp.spiht_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                ctypes.c_size_t]
    sp.log_set_quiet.argtypes = [ctypes.c_bool]
    sp.log_set_quiet(True)                                               # (the clamp to bits0 warns on every call)
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]

    def encode(img, tb):
        buf, n = ctypes.c_void_p(), ctypes.c_size_t()
        sp.spiht_encode(img.ctypes.data, img.shape[0], img.shape[1], ctypes.byref(buf), ctypes.byref(n), tb, 3)
        s = ctypes.string_at(buf.value, n.value)
        libc.free(buf)
        return s

    def decode(s, h, w, num_bits):
        b = ctypes.create_string_buffer(bytes(s), len(s))
        out = np.zeros((h, w), np.float32)
        sp.spiht_decode(b, len(s), out.ctypes.data, h, w, num_bits)
        return out

    return encode, decode


def _job(case):
    return S.digests(case, *_ref())


def main():
    assert os.path.exists(L.REF_SPIHT_SO), "needs the reference build (oracle/_ref)"
    with mp.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_job, S.CASES, chunksize=1)
    cases = {S.case_id(c): r for c, r in zip(S.CASES, res)}
    json.dump({"stream_bits": S.STREAM_BITS, "window": S.WINDOW, "cases": cases}, open(OUT, "w"), indent=0)
    print(len(cases), "cases,", sum(len(r["decode"]) + len(r["encode"]) for r in res), "digests,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
