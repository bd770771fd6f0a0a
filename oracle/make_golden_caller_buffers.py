#!/usr/bin/env python3
"""Golden hashes for the 721 x 1440 batch of tests/test_caller_buffers_gpu.py, written by the reference build
(oracle/_ref/libh5z_ebcc_ref.so).  TEST INFRASTRUCTURE; run in the dev container only:

    python3 oracle/make_golden_caller_buffers.py      ->  tests/golden/caller_buffers.json

Three frames (one that keeps its residual layer, a constant one, one whose base layer alone keeps the bound) in
MAX_ERROR, RELATIVE_ERROR and NONE with EBCC_INIT_BASE_ERROR_QUANTILE = 0.1: hashes only (input frame, stream, decoded
field) and what became of the residual layer.  The restated search of the oracle takes tens of seconds per frame at this
size, so the GPU test compares with these instead of running it."""
import ctypes
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _lib as L  # noqa: E402
from tests import test_caller_buffers_gpu as T  # noqa: E402

CONFIG = {"abs": (L.MAX_ERROR, 5.0, 0.01), "rel": (L.RELATIVE_ERROR, 5.0, 1e-4), "none": (L.NONE, 10.0, 0.0)}


def _job(job):
    name, k = job
    os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = T.QUANTILE
    mode, cr, err = CONFIG[name]
    x = T.big_frames()[k]
    cfg = L.make_config((1,) + T.BIG, base_cr=cr, error=err, residual_type=mode)
    s = L.ref_encode(x, cfg)
    assert s, "the reference wrote no stream"
    lib = L.reference()
    b = ctypes.create_string_buffer(s, len(s))
    out = ctypes.c_void_p()
    m = lib.ebcc_decode(b, len(s), ctypes.byref(out))
    assert m == x.size
    d = ctypes.string_at(out.value, 4 * m)
    lib.free_buffer(out)
    return {"field_sha256": T.sha(x.tobytes()), "n": len(s), "stream_sha256": T.sha(s), "decoded_sha256": T.sha(d),
            "kind": T.kind_of(s)}


def main():
    assert L.reference() is not None, "needs the reference build (oracle/_ref)"
    todo = [(name, k) for name in CONFIG for k in range(3)]
    with mp.get_context("spawn").Pool(min(9, os.cpu_count() or 1)) as pool:
        res = pool.map(_job, todo, chunksize=1)
    cases = {name: [r for (nm, _), r in zip(todo, res) if nm == name] for name in CONFIG}
    json.dump({"quantile": T.QUANTILE, "config": {k: [v[1], v[2]] for k, v in CONFIG.items()}, "cases": cases},
              open(os.path.join(L.GOLDEN, "caller_buffers.json"), "w"), indent=0)
    for name, rows in cases.items():
        print(name, [r["kind"] for r in rows])


if __name__ == "__main__":
    main()
