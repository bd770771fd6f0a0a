#!/usr/bin/env python3
"""Generate tests/golden/search_branches.json from the REFERENCE build for the case catalogue of tests/_domains.py.
Run in the dev container only:

    make -C oracle oracle ref && python oracle/make_golden_branches.py

For each case: the sha256 of its input field (the generators are deterministic; the hash catches a drift), the sha256
and length of the stream the reference build wrote, and the oracle's branch trace of the same encode (orc_last_trace:
which exits the two rate searches took, the residual outcome, the fallback flags).  The oracle's stream must equal the
reference's, or nothing is written.  The overflow case (max - min = inf) is recorded as refused: the reference stops
on an assert there, so it runs in a child process.  Test infrastructure; never imported by the product.
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _domains as D  # noqa: E402
from tests import _lib as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "search_branches.json")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def set_quantile(q):
    if q is None:
        os.environ.pop("EBCC_INIT_BASE_ERROR_QUANTILE", None)
    else:
        os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = q


def main():
    assert L.reference() is not None, "build the reference first: make -C oracle ref"
    L.oracle().orc_set_j2k_backend(0)
    cases = {}
    for c in D.catalogue():
        set_quantile(c.quantile)
        x = c.field()
        cfg = c.config(x)
        want = L.ref_encode(x, cfg)
        got = L.orc_encode(x, cfg)
        assert got == want, f"oracle != reference build for {c.name}"
        cases[c.name] = {"field_sha256": sha(x.tobytes()), "error": float(cfg.error), "n": len(want),
                         "stream_sha256": sha(want), "trace": L.trace()}
    set_quantile(None)
    o = D.overflow_case()
    cases[o.name] = {"field_sha256": sha(o.field().tobytes()), "error": float(o.config().error), "refused": True}
    assert D.reference_refuses(o), "the reference build no longer stops on the overflow case"
    json.dump({"cases": cases}, open(OUT, "w"), indent=0, sort_keys=True)
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
