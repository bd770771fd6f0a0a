"""The CPU oracle against the reference build at every bit budget and every cut of tests/_spiht_cuts.py.

tests/golden/spiht_cuts.json (oracle/make_golden_spiht_cuts.py) holds what the reference build's spiht_encode and spiht_decode
gave: a digest per 512 consecutive (num_bits, size) decodes and per 512 consecutive budgets.  The oracle reproduces every one,
so tests/test_spiht_cuts_gpu.py may take the live oracle as what the reference would give."""
import json
import os

import pytest

from tests import _lib as L
from tests import _spiht_cuts as S

with open(os.path.join(L.GOLDEN, "spiht_cuts.json")) as _f:
    GOLD = json.load(_f)


def test_fixture_matches_the_catalogue():
    assert GOLD["stream_bits"] == S.STREAM_BITS and GOLD["window"] == S.WINDOW
    assert list(GOLD["cases"]) == [S.case_id(c) for c in S.CASES]


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_oracle_reproduces_the_reference(case):
    h, w, name = case
    want = GOLD["cases"][S.case_id(case)]
    assert S.sha(S.image(h, w, name).tobytes()) == want["field_sha256"], "input differs"
    got = S.digests(case, L.orc_spiht_encode, L.orc_spiht_decode, S.threaded)
    assert (got["n"], got["stream_sha256"]) == (want["n"], want["stream_sha256"])
    pairs, budgets = S.decode_pairs(h, w, got["n"]), S.encode_budgets(h, w, name)
    assert len(got["decode"]) == len(want["decode"]) == -(-len(pairs) // S.WINDOW)
    assert len(got["encode"]) == len(want["encode"]) == -(-len(budgets) // S.WINDOW)
    bad = [(pairs[i * S.WINDOW], pairs[min(len(pairs), (i + 1) * S.WINDOW) - 1])
           for i, (a, b) in enumerate(zip(got["decode"], want["decode"])) if a != b]
    assert not bad, f"decodes differ in the windows of (num_bits, size) {bad}"
    bad = [(budgets[i * S.WINDOW], budgets[min(len(budgets), (i + 1) * S.WINDOW) - 1])
           for i, (a, b) in enumerate(zip(got["encode"], want["encode"])) if a != b]
    assert not bad, f"streams differ in the windows of trunc_bits {bad}"
