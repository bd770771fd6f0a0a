"""CPU: the frame-geometry catalogue of tests/_geometry.py.

1. What the catalogue covers, recomputed here from the rules themselves (integer arithmetic; neither the library nor the
   catalogue module's helpers), so that an edit of the catalogue shows what was lost:
   - a line of n samples has extent (n - 1) // 2^l + 1 at level l of the five-level 9/7, so the levels with an odd extent are
     given by (n - 1) mod 32;
   - the fused inverse level works on strips of 60 column pairs, four strips to a workgroup, and cuts the vertical positions of
     the top level into min(8, 256 // strips, ceil(H / 2) // 16) pieces (at least one);
   - the residual layer pads each axis to a multiple of 16, works on strips of 120 columns of the padded grid and cuts
     (ny / 2) // 16 pieces (at least one);
   - a plain frame takes the separate row and column passes at level 1 only where the coarsest band is one column wide: W = 32;
   - tile f of a chunk lies at row offset f h.
2. The oracle held to the reference at these shapes: tests/golden/geometry_sweep.json (oracle/make_golden_geometry.py: OpenJPEG
   2.4.0, the reference's residual coder, the reference build), and the programs themselves where oracle/_ref is present."""
import json
import os

import pytest

from tests import _geometry as G
from tests import _lib as L

FIXTURE = json.load(open(os.path.join(L.GOLDEN, "geometry_sweep.json")))


def ceil_div(a, b):
    return -(-a // b)


def top_pieces(h, w):
    strips = ceil_div(ceil_div(w, 2), 60)
    return max(1, min(8, 256 // strips, ceil_div(h, 2) // 16))


def last_strip(w):
    """(strips, column pairs in the last one, columns of its last pair) of the fused inverse top level"""
    pairs = ceil_div(w, 2)
    strips = ceil_div(pairs, 60)
    return strips, pairs - 60 * (strips - 1), 2 - w % 2


def pad(n):
    return -n % 16


def residual_pieces(h):
    return max(1, ((h + pad(h)) // 2) // 16)


def padded_last_strip(w):
    """frame columns in the last 120-column strip of the padded grid"""
    strips = ceil_div(w + pad(w), 120)
    return max(0, w - 120 * (strips - 1))


def coverage(plain, chunks):
    """-> the names of what the catalogue does not reach"""
    lost = []

    def need(what, ok):
        if not ok:
            lost.append(what)

    hs, ws = [s[0] for s in plain], [s[1] for s in plain]
    need("every pattern of odd levels over the heights", {(h - 1) % 32 for h in hs} == set(range(32)))
    need("every pattern of odd levels over the widths", {(w - 1) % 32 for w in ws} == set(range(32)))
    need("every pad of the heights", {pad(h) for h in hs} == set(range(16)))
    need("every pad of the widths", {pad(w) for w in ws} == set(range(16)))
    need("top-level pieces 1 .. 8", {top_pieces(h, w) for h, w in plain} >= set(range(1, 9)))
    need("residual pieces 1 .. 8", {residual_pieces(h) for h in hs} >= set(range(1, 9)))
    need("a last strip of one pair with one column", any(last_strip(w)[0] > 1 and last_strip(w)[1:] == (1, 1) for w in ws))
    need("a last strip of one pair with two columns", any(last_strip(w)[0] > 1 and last_strip(w)[1:] == (1, 2) for w in ws))
    # four strips to a workgroup: a fifth is a lone wave in a second workgroup, with one and with two columns
    need("a fifth strip of one column", any(last_strip(w) == (5, 1, 1) for w in ws))
    need("a fifth strip of two columns", any(last_strip(w) == (5, 1, 2) for w in ws))
    need("a padded last strip with 0 .. 4 frame columns", {padded_last_strip(w) for w in ws if w + pad(w) > 120} >= set(range(5)))
    need("three shapes of W = 32 with H != 32", sum(1 for h, w in plain if w == 32 and h != 32) >= 3)
    need("three shapes of H = 32 with W != 32", sum(1 for h, w in plain if h == 32 and w != 32) >= 3)
    need("32 and 64 on both axes", {32, 64} <= set(hs) and {32, 64} <= set(ws))
    need("legal frames", all(32 <= v <= 2047 for s in plain for v in s) and all(32 <= v <= 2047 for s in chunks for v in s[1:]))
    need("chunks of two frames", all(s[0] == 2 for s in chunks) and len(chunks) > 0)
    need("every offset mod 32 of the second tile", {s[1] % 32 for s in chunks if s[0] == 2} == set(range(32)))
    return lost


def test_the_catalogue_covers_what_it_is_for():
    assert coverage(G.PLAIN, G.D) == []
    assert len(G.PLAIN) == len(set(G.PLAIN)) == 52 and len(G.D) == len(set(G.D)) == 32
    # the figures stated with the catalogue
    assert [top_pieces(h, w) for h, w in G.B] == [1, 2, 2, 3, 4, 5, 6, 7, 7, 8, 1, 1, 1]
    assert [last_strip(w)[0] for _, w in G.B] == [1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 3, 5, 5]
    assert [last_strip(w)[1] for _, w in G.B] == [60, 60, 1, 1, 2, 2, 60, 60, 1, 1, 2, 1, 1]
    assert [last_strip(w)[2] for _, w in G.B[2:4] + G.B[8:10] + G.B[11:]] == [2, 1, 1, 2, 1, 2]
    assert [residual_pieces(h) for h, _ in G.B] == [2, 2, 3, 3, 4, 5, 6, 7, 8, 8, 1, 1, 1]
    assert [padded_last_strip(w) for _, w in G.B] == [0, 0, 2, 1, 3, 4, 119, 120, 1, 2, 3, 1, 2]
    assert sorted(h for h, _ in G.A) == sorted(w for _, w in G.A) == list(range(32, 65))


@pytest.mark.parametrize("family,lost", [("A", {"every pattern of odd levels over the heights", "every pattern of odd levels over the widths",
                                                 "every pad of the heights", "every pad of the widths", "32 and 64 on both axes"}),
                                         ("B", {"top-level pieces 1 .. 8", "residual pieces 1 .. 8", "a last strip of one pair with one column",
                                                "a last strip of one pair with two columns", "a fifth strip of one column",
                                                "a fifth strip of two columns", "a padded last strip with 0 .. 4 frame columns"}),
                                         ("C", {"three shapes of W = 32 with H != 32", "three shapes of H = 32 with W != 32"}),
                                         ("D", {"chunks of two frames", "every offset mod 32 of the second tile"})])
def test_a_family_taken_out_is_missed(family, lost):
    plain = [s for s in G.PLAIN if s not in G.FAMILIES[family]]
    chunks = [s for s in G.D if s not in G.FAMILIES[family]]
    assert set(coverage(plain, chunks)) == lost


def test_the_fixture_holds_every_shape_and_stage():
    plain = {"input_j2k", "input_residual", "input_codec", "j2k_streams", "j2k_decoded", "spiht_streams", "spiht_decoded", "codec_abs",
             "codec_rel"}
    assert FIXTURE["openjpeg"] == "2.4.0"
    assert set(FIXTURE["cases"]) == {G.shape_id(s) for s in G.PLAIN + G.D}
    for s in G.PLAIN:
        assert set(FIXTURE["cases"][G.shape_id(s)]) == plain, s
    for s in G.D:
        assert set(FIXTURE["cases"][G.shape_id(s)]) == {"input", "chunk_abs"}, s
    assert sum(len(c) for c in FIXTURE["cases"].values()) == 52 * 9 + 32 * 2
    # what stands behind the digests
    assert (52 * G.COUNTS["j2k"], 52 * G.COUNTS["spiht"], 52 * G.COUNTS["codec"], 32 * G.COUNTS["chunk"]) == (312, 312, 104, 32)


def _compare(shape, got, want, who):
    for k in sorted(want):
        if k.startswith("input"):
            assert got[k] == want[k], f"input differs: {G.shape_id(shape)} {k}"
    for k in sorted(want):
        assert got[k] == want[k], f"{who}: {G.shape_id(shape)} (family {G.family(shape)}): stage {k} differs"


@pytest.mark.parametrize("shape", G.PLAIN + G.D, ids=G.shape_id)
def test_oracle_equals_the_reference(shape, monkeypatch):
    """every stage digest of the shape: the oracle's is the one the reference's programs wrote, and the one they give now where
    they are present"""
    for k in G.ENV:
        monkeypatch.delenv(k, raising=False)
    want = FIXTURE["cases"][G.shape_id(shape)]
    try:
        got = G.all_digests(shape, G.oracle_coder())
        assert set(got) == set(want)
        _compare(shape, got, want, "the oracle against the fixture")
        lib = L.oracle()
        if L.reference() is not None and os.path.exists(L.REF_SPIHT_SO) and hasattr(lib, "orc_opj_encode") and L.opj_version() == FIXTURE["openjpeg"]:
            _compare(shape, G.all_digests(shape, G.reference_coder()), want, "the reference against the fixture")
    finally:
        L.oracle().orc_set_j2k_backend(0)
