#!/usr/bin/env python3
"""Golden digests over the frame-geometry catalogue of tests/_geometry.py, written by the reference build
(oracle/_ref/libh5z_ebcc_ref.so, oracle/_ref/libspiht_ref.so) and OpenJPEG 2.4.0 (the oracle's optional backend:
oracle/opj_backend.c).  TEST INFRASTRUCTURE; run in the dev container only, after a build:

    python3 oracle/make_golden_geometry.py      ->  tests/golden/geometry_sweep.json

One sha256 per shape and stage, taken over that shape's cases one after the other in the order of tests/_geometry.py
(digests, chunk_digests); per plain shape
- j2k_streams, j2k_decoded: OpenJPEG's codestreams and decoded samples of the three J2K frames at cr 1.0 and 12;
- spiht_streams, spiht_decoded: the reference coder's streams of the three residual frames at trunc_bits 0 and 8 (h w / 10),
  and its decode of the first third of each stream;
- codec_abs, codec_rel: ebcc_encode of the era5-like frame for MAX_ERROR at 1 % of the range and RELATIVE_ERROR 1e-3, base_cr 30;
per chunk of two frames
- chunk_abs: ebcc_encode for MAX_ERROR at 1 % of the range, base_cr 10;
and the sha256 of every input, so that a platform difference in an input fails as "input differs".  Digests only.

The oracle is run beside the reference on every shape and each one on which it departs is listed; the fixture is the
reference's either way.  tests/test_geometry_sweep.py holds the oracle to the file; tests/test_geometry_sweep_gpu.py compares
the product with the oracle."""
import json
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _geometry as G  # noqa: E402
from tests import _lib as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "geometry_sweep.json")


def _job(shape):
    G.clear_env()
    want = G.all_digests(shape, G.reference_coder())
    return want, sorted(k for k, v in G.all_digests(shape, G.oracle_coder()).items() if v != want[k])


def main():
    shapes = G.PLAIN + G.D
    with mp.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_job, shapes, chunksize=1)
    cases = {G.shape_id(s): r[0] for s, r in zip(shapes, res)}
    with open(OUT, "w") as f:
        json.dump({"openjpeg": L.opj_version(), "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(cases), "shapes,", sum(len(c) for c in cases.values()), "digests,", os.path.getsize(OUT), "bytes")
    departs = [f"{G.shape_id(s)}: {', '.join(r[1])}" for s, r in zip(shapes, res) if r[1]]
    if departs:
        print("THE ORACLE DEPARTS FROM THE REFERENCE in", len(departs), "shapes:", *departs, sep="\n  ")
        sys.exit(1)


if __name__ == "__main__":
    main()
