#!/usr/bin/env python3
"""Golden hashes for chunks of several frames whose tiles differ in geometry from position to position, written by the
reference build (oracle/_ref/libh5z_ebcc_ref.so: the reference's sources on OpenJPEG 2.4.0).  TEST INFRASTRUCTURE; run in
the dev container only, after a build:

    python3 oracle/make_golden_tiles.py      ->  tests/golden/tile_positions.json

The chunks are the catalogue of tests/_j2k_tables.py (CHUNKS under every rotation of the tile kinds, and the SPECIAL chunks):
formula inputs, of which only the sha256 is stored.  Per chunk
- mode NONE at every rate of tests/test_j2k_gpu.py: RATES, and
- for the catalogue chunks the BOUNDED modes (MAX_ERROR and RELATIVE_ERROR with a quantile and the pure-base fallback
  disabled, so that the residual layer over the stacked image stays and the chunk-level rate search runs),
each with the length and sha256 of the stream and the sha256 of the decoded field; the bounded cases also with coeffs_size
of the stream header.  tests/test_oracle_golden.py pins the oracle on all of them, tests/test_tile_positions_gpu.py the product.
The oracle is run beside the reference build and every case in which it departs is listed; the fixture is the reference's
either way."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _j2k_tables as T  # noqa: E402
from tests import _lib as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tile_positions.json")
RATES = [1.0, 3.0, 7.5, 30.0, 120.0, 1000.0]                            # tests/test_j2k_gpu.py: RATES (asserted by the tests)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def set_env(quantile):
    for k in T.BOUNDED_ENV:
        os.environ.pop(k, None)
    if quantile is not None:
        os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = quantile
        os.environ["EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK"] = "1"


def ref_decode(stream):
    lib = L.reference()
    b = ctypes.create_string_buffer(stream, len(stream))
    out = ctypes.c_void_p()
    m = lib.ebcc_decode(b, len(stream), ctypes.byref(out))
    assert m > 0, "the reference decoded nothing"
    d = ctypes.string_at(out.value, 4 * m)
    lib.free_buffer(out)
    return d


def run(x, cfg, departs, key):
    s = L.ref_encode(x, cfg)
    assert s, f"the reference wrote no stream for {key}"
    d = ref_decode(s)
    if L.orc_encode(x, cfg) != s or L.orc_decode(s).tobytes() != d:
        departs.append(key)
    return {"n": len(s), "stream_sha256": sha(s), "decoded_sha256": sha(d)}, s


def main():
    assert L.reference() is not None, "needs the reference build (oracle/_ref)"
    L.oracle().orc_set_j2k_backend(0)
    inputs, cases, departs = {}, {}, []
    for shape, kinds in T.fixture_chunks():
        x = T.chunk(kinds, *shape[1:])
        inputs[T.chunk_id(shape, kinds)] = sha(x.tobytes())
        set_env(None)
        for cr in RATES:
            key = T.rate_key(shape, kinds, cr)
            cases[key], _ = run(x, L.make_config(shape, base_cr=cr, error=0.0, residual_type=L.NONE), departs, key)
        for mode, err, base_cr, quantile in T.bounded_modes(shape, kinds):
            set_env(quantile)
            key = T.bounded_key(shape, kinds, mode)
            cases[key], s = run(x, L.make_config(shape, base_cr=base_cr, error=err, residual_type=mode), departs, key)
            cases[key]["coeffs_size"] = int.from_bytes(s[16:24], "little")
            assert cases[key]["coeffs_size"] > 0, f"{key}: no residual layer"
    set_env(None)
    json.dump({"openjpeg": L.opj_version(), "inputs": inputs, "cases": cases}, open(OUT, "w"), indent=0, sort_keys=True)
    print(len(inputs), "chunks,", len(cases), "cases,", os.path.getsize(OUT), "bytes")
    if departs:
        print("THE ORACLE DEPARTS FROM THE REFERENCE BUILD in", len(departs), "cases:", *departs, sep="\n  ")
        sys.exit(1)


if __name__ == "__main__":
    main()
