"""CPU tests: the oracle (oracle/*.c) against the committed golden vectors that were produced by the
reference build (oracle/make_golden.py), and - when that build is present (dev container) - directly
against it.  Bit-exact everywhere."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import _lib as L


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def load(name):
    return json.load(open(os.path.join(L.GOLDEN, name)))


@pytest.mark.parametrize("kat", load("spiht_kat.json"), ids=lambda k: f"{k['h']}x{k['w']}")
def test_spiht_known_answers(kat):
    img = L.kat_image(kat["h"], kat["w"])
    s = L.orc_spiht_encode(img, kat["trunc_bits"])
    assert len(s) == kat["n"]
    assert sha(s) == kat["stream_sha256"]
    if "stream_hex" in kat:
        assert s.hex() == kat["stream_hex"]
    dec = L.orc_spiht_decode(s, kat["h"], kat["w"])
    assert sha(dec.tobytes()) == kat["decoded_sha256"]


def test_survey_kat_prefixes():
    """SURVEY.md section 8(c) table (sha256 prefixes measured from the reference build)."""
    want = {(32, 32, 4096): ("6a538f1114869faa910aebb7", 528), (33, 47, 8192): ("ab343752056b65205b692fa8", 1040),
            (64, 64, 0): ("812a615043f9590d1beaad27", 4249)}
    for (h, w, tb), (pre, n) in want.items():
        s = L.orc_spiht_encode(L.kat_image(h, w), tb)
        assert len(s) == n and sha(s).startswith(pre)


def test_spiht_truncated_decode_edge_cases():
    img = L.smooth_image(40, 56, 1)
    s = L.orc_spiht_encode(img, 6000)
    for nbytes in (17, 18, 40, len(s) // 2, len(s)):
        d = L.orc_spiht_decode(s[:nbytes], 40, 56, 8 * nbytes)
        assert d.shape == (40, 56) and np.isfinite(d).all() and d.min() >= 0 and d.max() <= 1
    # monotone quality: the full stream is at least as good as a short prefix
    e_full = np.abs(L.orc_spiht_decode(s, 40, 56) - img).mean()
    e_short = np.abs(L.orc_spiht_decode(s[:40], 40, 56, 320) - img).mean()
    assert e_full <= e_short


_streams = load("codec_streams.json")
_inputs = np.load(os.path.join(L.GOLDEN, "codec_inputs.npz"))


@pytest.mark.parametrize("name", sorted(_streams), ids=str)
def test_frame_codec_streams(name, monkeypatch):
    c = _streams[name]
    if c["quantile"] is None:
        monkeypatch.delenv("EBCC_INIT_BASE_ERROR_QUANTILE", raising=False)
    else:
        monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", c["quantile"])
    L.oracle().orc_set_j2k_backend(0)
    cfg = L.make_config((1, c["h"], c["w"]), base_cr=c["base_cr"], error=c["error"], residual_type=c["mode"])
    want = bytes.fromhex(c["stream_hex"])
    got = L.orc_encode(_inputs[c["input"]], cfg)
    assert got == want
    dec = L.orc_decode(want)
    assert sha(dec.tobytes()) == c["decoded_sha256"]


_tiled = load("tiled.json")
_tiled_inputs = np.load(os.path.join(L.GOLDEN, "tiled_inputs.npz"))


@pytest.mark.parametrize("backend", [0, 1], ids=["restated-j2k", "openjpeg"])
@pytest.mark.parametrize("name", sorted(_tiled["frames"]), ids=str)
def test_multi_frame_chunk_streams(name, backend, monkeypatch):
    """Chunks of several frames: one tile per frame (reference src/ebcc_codec.c:105-180), including frame heights that
    put every tile at its own sub-band parity (the odd_* inputs)."""
    c = _tiled["frames"][name]
    for k in ("EBCC_INIT_BASE_ERROR_QUANTILE", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK"):
        monkeypatch.delenv(k, raising=False)
    if c["quantile"]:
        monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", c["quantile"].split("+")[0])
        if c["quantile"].endswith("+nofallback"):
            monkeypatch.setenv("EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "1")
    if backend == 1 and (not hasattr(L.oracle(), "orc_opj_version") or not L.opj_version()):
        pytest.skip("OpenJPEG backend not available on this machine")
    L.oracle().orc_set_j2k_backend(backend)
    try:
        x = _tiled_inputs[c["input"]]
        cfg = L.make_config(x.shape, base_cr=c["base_cr"], error=c["error"], residual_type=c["mode"])
        want = bytes.fromhex(c["stream_hex"])
        assert L.orc_encode(x, cfg) == want
        assert sha(L.orc_decode(want).tobytes()) == c["decoded_sha256"]
    finally:
        L.oracle().orc_set_j2k_backend(0)


def test_residual_branch_is_exercised():
    assert sum(1 for c in _streams.values() if c["coeffs_size"] > 0) >= 4


def _make_data(shape):
    idx = np.indices(shape, dtype=np.float32)
    return np.ascontiguousarray(idx[0] * 100.0 + idx[1] * 1.5 + idx[2] * 0.25, dtype=np.float32)


@pytest.mark.parametrize("name", sorted(load("ebck.json")), ids=str)
def test_ebck_containers(name):
    c = load("ebck.json")[name]
    shape, chunk = tuple(c["shape"]), tuple(c["chunk"])
    cfg = L.make_config(shape, chunk if any(chunk) else None, base_cr=2.0, error=c["error"], residual_type=c["mode"])
    L.oracle().orc_set_j2k_backend(0)
    s = L.orc_encode(_make_data(shape), cfg, "orc_" + c["fn"])
    assert len(s) == c["n"] and sha(s) == c["stream_sha256"]
    d = L.orc_decode(s, "orc_ebcc_decode_chunking")
    assert sha(d.tobytes()) == c["decoded_sha256"]
    # header fields, reference tests/test_c_api.py:182-188
    assert s[:4] == b"EBCK"
    ver, ndims = np.frombuffer(s[4:12], np.uint32)
    dims = tuple(int(v) for v in np.frombuffer(s[16:40], np.uint64))
    assert ver == 1 and ndims == 3 and dims == shape


@pytest.mark.parametrize("name", sorted(_tiled["ebck"]), ids=str)
def test_multi_frame_chunk_containers(name):
    """EBCK containers whose chunks hold several frames (reference tests/test_c_api.py:194-258 shapes plus frame heights
    that are not a multiple of 32)."""
    c = _tiled["ebck"][name]
    shape, chunk = tuple(c["shape"]), tuple(c["chunk"])
    cfg = L.make_config(shape, chunk if any(chunk) else None, base_cr=2.0, error=c["error"], residual_type=c["mode"])
    L.oracle().orc_set_j2k_backend(0)
    s = L.orc_encode(_make_data(shape), cfg, "orc_ebcc_encode_chunking")
    assert len(s) == c["n"] and sha(s) == c["stream_sha256"]
    assert sha(L.orc_decode(s, "orc_ebcc_decode_chunking").tobytes()) == c["decoded_sha256"]


@pytest.mark.parametrize("name", sorted(_tiled["big"]), ids=str)
def test_multi_frame_chunk_extremes(name):
    """Two ERA5-sized frames per chunk, the most tiles a chunk can hold (63), the tallest tiles (1023 rows): formula
    inputs, hashes from the reference build."""
    c = _tiled["big"][name]
    shape = tuple(c["shape"])
    cfg = L.make_config(shape, base_cr=c["base_cr"], error=c["error"], residual_type=c["mode"])
    L.oracle().orc_set_j2k_backend(0)
    s = L.orc_encode(L.formula_frames(*shape), cfg)
    assert len(s) == c["n"] and sha(s) == c["stream_sha256"]
    assert sha(L.orc_decode(s).tobytes()) == c["decoded_sha256"]


_tiles = load("tile_positions.json")


def _tile_chunks():
    from tests import _j2k_tables as T
    return T.fixture_chunks()


@pytest.mark.parametrize("backend", [0, 1], ids=["restated-j2k", "openjpeg"])
@pytest.mark.parametrize("shape,kinds", _tile_chunks(), ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else "+".join(v))
def test_tile_position_chunk_streams(shape, kinds, backend, monkeypatch):
    """Chunks whose tiles differ in geometry from position to position (sub-band parities, a first code-block row of 1 to 63
    lines, more code-blocks at one position than at another) with hostile content in every tile, over the rate ladder and
    in both bounded modes: streams and decoded fields of the reference build (oracle/make_golden_tiles.py)."""
    from tests import _j2k_tables as T
    from tests.test_j2k_gpu import RATES
    if backend == 1 and (not hasattr(L.oracle(), "orc_opj_version") or not L.opj_version()):
        pytest.skip("OpenJPEG backend not available on this machine")
    x = T.chunk(kinds, *shape[1:])
    assert sha(x.tobytes()) == _tiles["inputs"][T.chunk_id(shape, kinds)], "input differs"
    jobs = [(T.rate_key(shape, kinds, cr), None, L.make_config(shape, base_cr=cr, error=0.0, residual_type=L.NONE)) for cr in RATES]
    jobs += [(T.bounded_key(shape, kinds, mode), q, L.make_config(shape, base_cr=base_cr, error=err, residual_type=mode))
             for mode, err, base_cr, q in T.bounded_modes(shape, kinds)]
    L.oracle().orc_set_j2k_backend(backend)
    try:
        for key, quantile, cfg in jobs:
            c = _tiles["cases"][key]
            for k in T.BOUNDED_ENV:
                monkeypatch.delenv(k, raising=False)
            if quantile is not None:
                monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", quantile)
                monkeypatch.setenv("EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "1")
            s = L.orc_encode(x, cfg)
            assert len(s) == c["n"] and sha(s) == c["stream_sha256"], key
            assert sha(L.orc_decode(s).tobytes()) == c["decoded_sha256"], key
            if "coeffs_size" in c:
                assert int.from_bytes(s[16:24], "little") == c["coeffs_size"] > 0, key
    finally:
        L.oracle().orc_set_j2k_backend(0)


def test_tile_position_fixture_holds_every_case():
    from tests import _j2k_tables as T
    from tests.test_j2k_gpu import RATES
    want = {T.rate_key(s, k, cr) for s, k in T.fixture_chunks() for cr in RATES}
    want |= {T.bounded_key(s, k, b[0]) for s, k in T.fixture_chunks() for b in T.bounded_modes(s, k)}
    assert set(_tiles["cases"]) == want and len(want) == 38 * 6 + 8 * 2
    assert set(_tiles["inputs"]) == {T.chunk_id(s, k) for s, k in T.fixture_chunks()}
    assert _tiles["openjpeg"] == "2.4.0"


_live = load("live_checks.json")
_live_inputs = np.load(os.path.join(L.GOLDEN, "live_checks_inputs.npz"))


def test_j2k_restatement_matches_openjpeg_live():
    """The restated encoder against OpenJPEG 2.4.0 on small natural-looking images: the codestreams OpenJPEG wrote
    (oracle/make_golden_live.py), and OpenJPEG itself where the oracle's backend finds the library."""
    lib = L.oracle()
    live = hasattr(lib, "orc_opj_encode") and L.opj_version() == _live["openjpeg"]

    def enc(fn, img, cr):
        out = ctypes.c_void_p()
        n = fn(img.ctypes.data, img.shape[0], img.shape[1], ctypes.c_float(cr), ctypes.byref(out))
        s = ctypes.string_at(out.value, n)
        lib.orc_free(out)
        return s

    for c in _live["opj"]:
        img = np.ascontiguousarray(_live_inputs[c["input"]])
        s = enc(lib.orc_j2k_encode, img, c["cr"])
        assert len(s) == c["n"] and sha(s) == c["stream_sha256"], (c["input"], c["cr"])
        if live:
            assert enc(lib.orc_opj_encode, img, c["cr"]) == s, (c["input"], c["cr"])


_j2k = json.load(open(os.path.join(L.GOLDEN, "j2k_openjpeg.json")))
_j2k_inputs = np.load(os.path.join(L.GOLDEN, "j2k_inputs.npz"))
# the high-entropy fields at the large and thin shapes (oracle/make_golden_j2k.py fields): the cases marked "pin"
_j2k_cases = _j2k["cases"] + [c for c in load("j2k_fields.json")["cases"] if c["pin"]]


def _j2k_input(c):
    if "kind" in c:
        from tests import _fields as F
        x = F.field(c["kind"], c["h"], c["w"])
        assert sha(x.tobytes()) == c["field_sha256"], "input differs"
        return L.scale_u16(x)[0]
    if c["input"] == "stored":
        return np.ascontiguousarray(_j2k_inputs[c["spec"]])
    h, w, k = c["spec"]
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    v = (x * x * 3 + y * y * 5 + x * y * (k + 1)) % 4096 * 12 + ((x // 16) * 7 + (y // 16) * 13 + k) % 97 * 160 + (x * 7 + y * 13) % 31
    return np.ascontiguousarray((v % 65536).astype(np.uint16))


@pytest.mark.parametrize("i", range(len(_j2k_cases)),
                         ids=lambda i: ("{h}x{w}-{kind}-cr{cr}" if "kind" in _j2k_cases[i] else "{h}x{w}-cr{cr}").format(**_j2k_cases[i]))
def test_j2k_restatement_against_openjpeg_fixtures(i):
    """oracle/j2k_oracle.c (the restated JPEG 2000 base layer) against codestreams and decoded samples produced by the real
    OpenJPEG 2.4.0 through the reference's call sequence (oracle/make_golden_j2k.py; /root/reference/src/ebcc_codec.c:105-180,
    :1092-1136): byte-identical codestream, identical decoded samples - on any box, with or without the library.  The
    field cases also pin the samples mapped back to float32, which the GPU tests compare with."""
    c = _j2k_cases[i]
    img = _j2k_input(c)
    s = L.orc_j2k_encode(img, c["cr"])
    assert len(s) == c["n"] and sha(s) == c["stream_sha256"]
    if "stream_hex" in c:
        assert s == bytes.fromhex(c["stream_hex"])
    samples = L.orc_j2k_decode(s)
    assert sha(samples.tobytes()) == c["decoded_sha256"]
    if "mapped_sha256" in c:
        from tests import _fields as F
        _, mn, mx = L.scale_u16(F.field(c["kind"], c["h"], c["w"]))
        assert sha(L.map_decoded(samples, mn, mx).tobytes()) == c["mapped_sha256"]


def test_j2k_nmsedec_tables_match_openjpeg_binary_dump():
    """Spot values read from the rodata of libopenjp2 2.4.0 (lut_nmsedec_*), kept as literals."""
    lib = L.oracle()
    lib.orc_j2k_lut.restype = ctypes.POINTER(ctypes.c_int16)
    sig = [lib.orc_j2k_lut(0)[i] for i in range(128)]
    sig0 = [lib.orc_j2k_lut(1)[i] for i in range(128)]
    ref = [lib.orc_j2k_lut(2)[i] for i in range(128)]
    ref0 = [lib.orc_j2k_lut(3)[i] for i in range(128)]
    assert sig[:20] == [0] * 20 and sig[-6:] == [28416, 28800, 29184, 29568, 29952, 30336]
    assert sig0[:20] == [0, 0, 0, 0, 0, 0, 128, 128, 128, 128, 256, 256, 256, 384, 384, 512, 512, 640, 640, 768]
    assert sig0[-6:] == [29824, 30208, 30720, 31232, 31744, 32256]
    assert ref[:4] == [6144, 6016, 5888, 5760] and ref[-6:] == [5376, 5504, 5632, 5760, 5888, 6016]
    assert ref0[:4] == [8192, 7936, 7680, 7424] and ref0[-6:] == [6784, 6912, 7168, 7424, 7680, 7936]


def test_legacy_repack_is_what_the_reference_decodes():
    """tests/_lib.legacy_repack (used by the GPU legacy-stream test) against the oracle's ebcc_decode_legacy
    restatement and, in the dev container, the reference build itself."""
    import hashlib
    import json
    streams = json.load(open(os.path.join(L.GOLDEN, "codec_streams.json")))
    names = sorted(streams)[::9]
    ref = None
    if os.path.exists(L.REF_SO):
        ref = ctypes.CDLL(L.REF_SO)
        ref.ebcc_decode.restype = ctypes.c_size_t
        ref.ebcc_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, L.c_void_pp]
    for name in names:
        s = bytes.fromhex(streams[name]["stream_hex"])
        leg = L.legacy_repack(s)
        dec = L.orc_decode(leg)
        assert hashlib.sha256(np.asarray(dec, np.float32).tobytes()).hexdigest() == streams[name]["decoded_sha256"], name
        if ref is not None:
            b = ctypes.create_string_buffer(leg, len(leg))
            out = ctypes.c_void_p()
            n = ref.ebcc_decode(b, len(leg), ctypes.byref(out))
            got = np.frombuffer(ctypes.string_at(out.value, 4 * n), np.float32)
            assert hashlib.sha256(got.tobytes()).hexdigest() == streams[name]["decoded_sha256"], name


ENV_SWITCHES = ["EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK_CONSISTENCY",
                "EBCC_DISABLE_MEAN_ADJUSTMENT"]


def env_switch_cases(switch):
    """(frame, config, what the reference build wrote) triples that exercise both outcomes of the :838 selection
    (residual kept / pure base layer); frames stored with the reference's streams (oracle/make_golden_live.py)."""
    return [(np.ascontiguousarray(_live_inputs[c["input"]], np.float32),
             L.make_config(tuple(c["shape"]), base_cr=c["base_cr"], error=c["error"], residual_type=c["mode"]), c)
            for c in _live["env_switches"][switch]]


@pytest.mark.parametrize("switch", ENV_SWITCHES)
def test_oracle_env_switches_match_reference(switch, monkeypatch):
    """The three EBCC_DISABLE_* switches of src/ebcc_codec.c:634-649: oracle == reference build (its streams as stored,
    and the build itself where it is present), so that the GPU test of the same switches (tests/test_codec_gpu.py) can
    use the oracle on a box without the reference."""
    ref = None
    if os.path.exists(L.REF_SO):
        ref = ctypes.CDLL(L.REF_SO)
        ref.ebcc_encode.restype = ctypes.c_size_t
        ref.ebcc_encode.argtypes = [ctypes.c_void_p, ctypes.POINTER(L.CodecConfig), L.c_void_pp]
    monkeypatch.setenv(switch, "1")
    monkeypatch.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", _live["env_quantile"])   # loose base layer: the switches change the streams
    for frame, cfg, c in env_switch_cases(switch):
        s = L.orc_encode(frame, cfg)
        assert len(s) == c["n"] and sha(s) == c["stream_sha256"], (switch, c["input"], c["mode"])
        if ref is not None:
            out = ctypes.c_void_p()
            n = ref.ebcc_encode(frame.ctypes.data, ctypes.byref(cfg), ctypes.byref(out))
            assert ctypes.string_at(out.value, n) == s, switch


_branches = load("search_branches.json")["cases"]


def test_search_branch_streams():
    """The catalogue of tests/_domains.py (value domains x error targets x start rates x quantiles): oracle streams ==
    the reference build's as stored (oracle/make_golden_branches.py), inputs as generated when the fixture was made."""
    from tests import _domains as D
    L.oracle().orc_set_j2k_backend(0)
    old = os.environ.pop("EBCC_INIT_BASE_ERROR_QUANTILE", None)
    try:
        for c in D.catalogue():
            want = _branches[c.name]
            if c.quantile is not None:
                os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = c.quantile
            x = c.field()
            assert sha(x.tobytes()) == want["field_sha256"], c.name
            s = L.orc_encode(x, c.config(x))
            os.environ.pop("EBCC_INIT_BASE_ERROR_QUANTILE", None)
            assert len(s) == want["n"] and sha(s) == want["stream_sha256"], c.name
    finally:
        if old is not None:
            os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = old


_large = load("large_frames.json")
# the oracle's restated search takes tens of seconds per full-size frame of noise: it is pinned on the frames it codes in
# a few seconds (the reference build on the same ones, where it is present); the GPU module compares every case
_LARGE_SAMPLE = [("batch_1024", ("spike", 0)), ("batch_1024", ("checker", 0)), ("batch_1024", ("lowbit", 0)),
                 ("batch_2047", ("spike", 2))]


def test_large_frame_inputs():
    """Every input of tests/golden/large_frames.json is the frame the generators make here."""
    from tests import _fields as F
    for batch, ((h, w), specs) in F.LARGE_BATCHES.items():
        for spec in specs:
            x = F.large_frame(spec[0], h, w, spec[1])
            for mode, _ in F.LARGE_MODES:
                assert sha(x.tobytes()) == _large["cases"][F.large_key(batch, spec, mode)]["field_sha256"], (batch, spec)
    for mode, _ in F.EXTREME_MODES:
        assert sha(F.extreme_frame().tobytes()) == _large["cases"][F.large_key("extreme", None, mode)]["field_sha256"]
    for mode, _ in F.LARGE_MODES:
        assert sha(F.compat_array().tobytes()) == _large["cases"][F.large_key("compat", None, mode)]["field_sha256"]


@pytest.mark.parametrize("mode,err", [(L.MAX_ERROR, 0.05), (L.RELATIVE_ERROR, 1e-3)], ids=["abs", "rel"])
@pytest.mark.parametrize("batch,spec", _LARGE_SAMPLE, ids=lambda v: v if isinstance(v, str) else "{}{}".format(*v))
def test_large_frame_streams(batch, spec, mode, err, monkeypatch):
    """oracle == the reference build's stream and decoded field at 1024 x 1024 and 2047 x 2047 (as stored, and the
    build itself where it is present)."""
    from tests import _fields as F
    monkeypatch.delenv("EBCC_INIT_BASE_ERROR_QUANTILE", raising=False)
    assert (mode, err) in F.LARGE_MODES
    (h, w), _ = F.LARGE_BATCHES[batch]
    c = _large["cases"][F.large_key(batch, spec, mode)]
    x = F.large_frame(spec[0], h, w, spec[1])
    cfg = L.make_config((1, h, w), base_cr=_large["base_cr"], error=err, residual_type=mode)
    L.oracle().orc_set_j2k_backend(0)
    s = L.orc_encode(x, cfg)
    assert len(s) == c["n"] and sha(s) == c["stream_sha256"]
    assert sha(L.orc_decode(s).tobytes()) == c["decoded_sha256"]
    if L.reference() is not None:
        assert L.ref_encode(x, cfg) == s


@pytest.mark.parametrize("i", range(len(_large["spiht"])),
                         ids=lambda i: "{h}x{w}-{kind}-tb{trunc_bits}".format(**_large["spiht"][i]))
def test_spiht_large_fields(i):
    """The residual coder at 1024 x 1024, 2047 x 2047 and 2047 x 33 on noise, spike and checkerboard images, untruncated
    and truncated: oracle == the reference build (as stored, and the build itself where it is present)."""
    from tests import _fields as F
    c = _large["spiht"][i]
    h, w = c["h"], c["w"]
    x = F.field(c["kind"], h, w, c["seed"])
    assert sha(x.tobytes()) == c["field_sha256"], "input differs"
    s = L.orc_spiht_encode(x, c["trunc_bits"])
    assert len(s) == c["n"] and sha(s) == c["stream_sha256"]
    assert c["trunc_bits"] or len(s) <= h * w * 4                    # the reference's buffer when untruncated
    assert sha(L.orc_spiht_decode(s, h, w).tobytes()) == c["decoded_sha256"]
    if os.path.exists(L.REF_SPIHT_SO):
        sp = ctypes.CDLL(L.REF_SPIHT_SO)
        sp.spiht_encode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, L.c_void_pp, L.c_size_p,
                                    ctypes.c_size_t, ctypes.c_size_t]
        buf, n = ctypes.c_void_p(), ctypes.c_size_t()
        sp.spiht_encode(x.ctypes.data, h, w, ctypes.byref(buf), ctypes.byref(n), c["trunc_bits"], 3)
        assert ctypes.string_at(buf.value, n.value) == s
