"""GPU: results must not depend on what device memory holds when a call starts.

Poisoned workspace: each (pattern, group) cell runs its cases in a fresh child process with EBCC_HIP_POISON_ALLOC set,
so every float / double workspace buffer and every byte buffer that ends up in a stream starts as 0xFF bytes (NaN) or
0x7F bytes (3.4e38 / 1.4e306) instead of the zeros of a fresh allocation.  A kernel that reads such a buffer where it
did not write in the call gives a wrong number, and the case fails against the fixture the existing tests check it
with.  Every group holds partial batches (fewer frames than the context holds), whose idle slots no call writes.

History: the same engines run a harsher workload first (deep SPIHT, long searches, full code-block slots, a larger
batch, engines re-made by the public API), so their memory holds real, in-range data from an earlier call; the calls
that follow must still give the fixture's or the oracle's bytes."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest

from tests import _domains as D
from tests import _fields as F
from tests import _lib as L
from tests import test_codec_gpu as C
from tests import test_j2k_gpu as J
from tests import test_large_frames_gpu as LF
from tests import test_residual_gpu as R
from tests import test_search_branches_gpu as S

pytestmark = pytest.mark.gpu

PATTERNS = {"0xFF": 1, "0x7F": 1}          # pattern -> every k-th case of each group
GROUPS = ("single", "chunks", "search", "kernels", "large", "decode")
SEARCH_ENV = ("EBCC_INIT_BASE_ERROR_QUANTILE", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK", "EBCC_DISABLE_MEAN_ADJUSTMENT")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


class _Env:
    """monkeypatch's setenv / delenv on the child's own environment (the library reads these at every call)"""

    @staticmethod
    def setenv(k, v):
        os.environ[k] = v

    @staticmethod
    def delenv(k, raising=True):
        os.environ.pop(k, None)


def _default_env():
    for k in SEARCH_ENV:
        os.environ.pop(k, None)


# ---- case groups: (name, thunk) lists; a thunk raises when its case is wrong ----------------------------------
def _single_cases():
    """all golden single-frame streams through ebcc_encode / ebcc_decode, then the same case as a 1-frame batch of a
    context of 3 frames per shape (slots 1 and 2 are never written)"""
    ctxs = {}

    def partial(name):
        c = C._streams[name]
        if (c["h"], c["w"]) not in ctxs:
            ctxs[(c["h"], c["w"])] = L.Context(3, c["h"], c["w"])
        ctx = ctxs[(c["h"], c["w"])]
        cfg = L.make_config((1, c["h"], c["w"]), base_cr=c["base_cr"], error=c["error"], residual_type=c["mode"])
        want = bytes.fromhex(c["stream_hex"])
        assert ctx.encode_frames(C._inputs[c["input"]][None], cfg)[0] == want, "partial batch: stream"
        assert sha(ctx.decode_frames([want])[0].tobytes()) == c["decoded_sha256"], "partial batch: decode"

    def case(name):
        C.test_golden_streams_bit_exact(name, _Env)           # (sets the case's quantile)
        partial(name)

    return [(f"golden/{n}", lambda n=n: case(n)) for n in sorted(C._streams)]


def _chunk_cases():
    """tiled.json frames and ebck, ebck.json: the largest chunk counts first, so that later calls on the same geometry
    run as partial batches of engines made for more frames"""
    def size(shape):
        return int(np.prod(shape))

    cases = []
    for n, c in C._tiled["frames"].items():
        cases.append((size(C._tiled_inputs[c["input"]].shape), f"tiled-frames/{n}",
                      lambda n=n: C.test_multi_frame_chunks_bit_exact(n, _Env)))
    for n, c in C._tiled["ebck"].items():
        cases.append((size(c["shape"]), f"tiled-ebck/{n}", lambda n=n: C.test_multi_frame_chunk_containers_bit_exact(n)))
    for n, c in C._ebck.items():
        cases.append((size(c["shape"]), f"ebck/{n}", lambda n=n: C.test_ebck_containers_bit_exact(n)))
    return [(name, fn) for _, name, fn in sorted(cases, key=lambda t: (-t[0], t[1]))]


def _search_groups():
    g = defaultdict(list)
    for c in D.catalogue():
        g[(c.shape, c.quantile)].append(c)
    return sorted(g.items(), key=lambda kv: (kv[0][0], kv[0][1] or ""))


def _mixed_batch(shape, quantile, cases):
    """every field of the group under one MAX_ERROR case's config, in a context 3 frames larger than the batch: that
    case's frame is the reference's stream, every other frame the product's single-frame stream of the same input, and
    decode_frames gives the oracle's decode"""
    _default_env()
    if quantile is not None:
        os.environ["EBCC_INIT_BASE_ERROR_QUANTILE"] = quantile
    lead = next(c for c in cases if c.mode == L.MAX_ERROR)
    fields = [c.field() for c in cases]
    cfg = lead.config(fields[cases.index(lead)])
    with L.Context(len(cases) + 3, *shape) as ctx:
        got = ctx.encode_frames(np.stack(fields), cfg)
        dec = ctx.decode_frames(got)
    assert sha(got[cases.index(lead)]) == S.FIXTURE[lead.name]["stream_sha256"], S._why(lead)
    for k, s in enumerate(got):
        assert s == S.encode(fields[k], cfg), ("partner", cases[k].name)
        assert S.same_bits(dec[k].ravel(), L.orc_decode(s)), ("decode", cases[k].name)


def _search_cases():
    out = [(f"catalogue/{c.name}", lambda c=c: S.test_single_frame_streams_and_fields(c, _Env)) for c in D.catalogue()]
    for (shape, q), cases in _search_groups():
        out.append((f"mixed/{shape[0]}x{shape[1]}-q{q or 'default'}", lambda s=shape, q=q, c=cases: _mixed_batch(s, q, c)))
    return out


def _j2k_smooth(h, w):
    """the smooth fields of test_j2k_gpu at three rates as a 3-frame batch of a 5-frame context: codestreams and true
    decode against the oracle"""
    fields = J._fields(h, w)
    with L.Context(len(fields) + 2, h, w) as ctx:
        for cr in (1.0, 7.5, 120.0):
            got, mm = ctx.j2k_encode(fields, [cr] * len(fields))
            dec = ctx.j2k_decode(got, mm)
            for f, fld in enumerate(fields):
                u16, mn, mx = L.scale_u16(fld)
                assert mm[f, 0] == mn and mm[f, 1] == mx, (cr, f)
                ref = L.orc_j2k_encode(u16, cr)
                assert got[f] == ref, (cr, f, "codestream")
                assert np.array_equal(dec[f], L.map_decoded(L.orc_j2k_decode(ref), mn, mx)), (cr, f, "decode")


def _j2k_field(kind):
    """a high-entropy 257 x 383 field at every rate of the ladder, 6 frames of an 8-frame context: OpenJPEG's codestreams
    and decoded samples (tests/golden/j2k_fields.json)"""
    h, w = 257, 383
    with L.Context(len(J.RATES) + 2, h, w) as ctx:
        _, streams, mm, want = J._field_streams(ctx, h, w, kind)
        got = ctx.j2k_decode(streams, [mm] * len(J.RATES))
    for i, c in enumerate(want):
        assert sha(got[i].tobytes()) == c["mapped_sha256"], (kind, c["cr"])


def _spiht(h, w):
    """the residual layer on the images of test_residual_gpu, a 7-frame batch of a 9-frame context: coefficients,
    streams at two budgets and decode against the oracle"""
    imgs = R._images(h, w)
    with L.Context(len(imgs) + 2, h, w) as ctx:
        c, dc = ctx.spiht_coeffs(imgs)
        for f, img in enumerate(imgs):
            ref, rdc = L.orc_spiht_coeffs(img)
            assert dc[f] == rdc and np.array_equal(c[f].reshape(ref.shape), ref), ("coeffs", f)
        for tb in (0, 8 * (h * w // 20)):
            got = ctx.spiht_encode(imgs, [tb] * len(imgs))
            for f, img in enumerate(imgs):
                assert got[f] == L.orc_spiht_encode(img, tb), ("stream", tb, f)
        streams = [L.orc_spiht_encode(img, 8 * (h * w // 10)) for img in imgs]
        dec = ctx.spiht_decode(streams)
        for f, s in enumerate(streams):
            assert np.array_equal(dec[f], L.orc_spiht_decode(s, h, w)), ("decode", f)


def _kernel_cases():
    out = [(f"j2k/{h}x{w}", lambda h=h, w=w: _j2k_smooth(h, w)) for h, w in ((33, 47), (100, 130), (181, 360))]
    out += [(f"j2k/257x383-{k}", lambda k=k: _j2k_field(k)) for k in ("noise", "checker")]
    out += [(f"spiht/{h}x{w}", lambda h=h, w=w: _spiht(h, w)) for h, w in ((33, 47), (100, 130), (37, 2047))]
    return out


def _full_size_partial():
    """the 721 x 1440 formula frame as a 1-frame batch of a 2-frame context, every config of codec_big.json"""
    big = json.load(open(os.path.join(L.GOLDEN, "codec_big.json")))
    f1 = C.full_size_formula_frame()
    with L.Context(2, 721, 1440) as ctx:
        for key, c in big.items():
            cfg = L.make_config((1, 721, 1440), base_cr=c["base_cr"], error=c["error"], residual_type=c["mode"])
            s = ctx.encode_frames(f1[None], cfg)[0]
            assert len(s) == c["n"] and sha(s) == c["stream_sha256"], key
            assert sha(ctx.decode_frames([s])[0].tobytes()) == c["decoded_sha256"], key


def _large_cases():
    out = [(f"batch_1024/{LF.MODE_IDS[m]}", lambda m=m, e=e: LF.test_batch_streams_and_fields("batch_1024", m, e))
           for m, e in F.LARGE_MODES]
    out.append(("formula_721x1440", C.test_full_size_formula_frames_bit_exact))
    out.append(("formula_721x1440/partial", _full_size_partial))
    return out


def _decode_batches(shape, names, sizes):
    """golden streams of one shape decoded in batches of the given sizes by a context larger than any of them, in a
    process where nothing was encoded"""
    with L.Context(max(sizes) + 2, *shape) as ctx:
        i = 0
        for k in sizes:
            part = names[i:i + k]
            dec = ctx.decode_frames([bytes.fromhex(C._streams[n]["stream_hex"]) for n in part])
            for n, d in zip(part, dec):
                assert sha(d.tobytes()) == C._streams[n]["decoded_sha256"], n
            i += k
        assert i == len(names)


def _container_decode(c):
    """the oracle's container of a chunking case (the reference's bytes: checked) through ebcc_decode_chunking"""
    shape, chunk = tuple(c["shape"]), tuple(c["chunk"])
    cfg = L.make_config(shape, chunk if any(chunk) else None, base_cr=2.0, error=c["error"], residual_type=c["mode"])
    L.oracle().orc_set_j2k_backend(0)
    s = L.orc_encode(C._make_data(shape), cfg, "orc_" + c.get("fn", "ebcc_encode_chunking"))
    assert sha(s) == c["stream_sha256"], "oracle container differs from the fixture"
    assert sha(C.api_decode(s, "ebcc_decode_chunking").tobytes()) == c["decoded_sha256"]


def _decode_cases():
    by_shape = defaultdict(list)
    for n, c in sorted(C._streams.items()):
        by_shape[(c["h"], c["w"])].append(n)
    out = []
    for shape, names in sorted(by_shape.items()):
        sizes = [1] + [3] * ((len(names) - 1) // 3) + ([(len(names) - 1) % 3] if (len(names) - 1) % 3 else [])
        out.append((f"frames/{shape[0]}x{shape[1]}", lambda s=shape, n=names, z=sizes: _decode_batches(s, n, z)))
    conts = sorted(list(C._ebck.items()) + list(C._tiled["ebck"].items()), key=lambda kv: (-int(np.prod(kv[1]["shape"])), kv[0]))
    out += [(f"chunking/{n}", lambda c=c: _container_decode(c)) for n, c in conts]
    return out


CASES = {"single": _single_cases, "chunks": _chunk_cases, "search": _search_cases, "kernels": _kernel_cases,
         "large": _large_cases, "decode": _decode_cases}


def _run_child(group, every):
    """(in the child) every `every`-th case of the group; one JSON line of {case: "ok" | what went wrong}"""
    res = {}
    for name, fn in CASES[group]()[::every]:
        _default_env()                                          # (what pytest's monkeypatch undoes after every test)
        try:
            fn()
            res[name] = "ok"
        except Exception as e:                                  # (AssertionError above all: the case is wrong)
            res[name] = f"{type(e).__name__}: {e}"[:400]
    print("WORKSPACE_RESULTS " + json.dumps(res), flush=True)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_poisoned_workspace(pattern, group):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EBCC_")}
    env["EBCC_HIP_POISON_ALLOC"] = pattern
    code = f"import sys; sys.path.insert(0, {L.ROOT!r}); from tests import test_workspace_gpu as W; W._run_child({group!r}, {PATTERNS[pattern]})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=L.ROOT, timeout=600)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stderr[-3000:]}"
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("WORKSPACE_RESULTS ")]
    assert len(line) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(line[0].split(" ", 1)[1])
    assert len(res) == len(CASES[group]()[::PATTERNS[pattern]])
    failed = {k: v for k, v in res.items() if v != "ok"}
    assert not failed, f"{len(failed)} of {len(res)} cases differ under {pattern}: " + json.dumps(failed, indent=1)


# ---- history independence: engines whose memory holds an earlier, harsher call's data --------------------------
HOSTILE_CFG = dict(base_cr=2.0, error=1e-3, residual_type=L.MAX_ERROR)


@pytest.fixture
def _clean_env(monkeypatch):
    for k in SEARCH_ENV + ("EBCC_HIP_SLICES", "EBCC_HIP_DECODE_SLICES", "EBCC_HIP_MAX_BATCH"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_same_context_after_hostile_frames(_clean_env):
    """H1: one 100 x 130 context of 8 frames.  8 hostile frames (noise, checker, spike at base_cr 2 and 1e-3: deep
    SPIHT, long truncation searches, full code-block slots), then the in2 / in3 golden cases as 1- and 2-frame batches
    (modes and quantiles cycling), then the hostile streams decoded, then the golden streams as 1- and 3-frame batches."""
    mp = _clean_env
    h, w = 100, 130
    hostile = np.stack([F.field(k, h, w, s) for k, s in (("noise", 0), ("noise", 1), ("noise", 2), ("checker", 0),
                                                         ("checker", 1), ("spike", 0), ("spike", 1), ("checker", 2))])
    golden = defaultdict(list)                                  # one config -> its in2 and in3 cases
    for n, c in C._streams.items():
        if c["input"] in ("in2", "in3"):
            golden[(c["base_cr"], c["error"], c["quantile"] or "", c["mode"])].append(n)
    keys = sorted(golden, key=lambda k: (k[0], k[1], k[2], k[3]))
    assert len(keys) == 18 and all(len(golden[k]) == 2 for k in keys)
    with L.Context(8, h, w) as ctx:
        hcfg = L.make_config((1, h, w), **HOSTILE_CFG)
        hs = ctx.encode_frames(hostile, hcfg)
        for i, k in enumerate(keys):
            names = sorted(golden[k])
            c = C._streams[names[0]]
            if c["quantile"] is None:
                mp.delenv("EBCC_INIT_BASE_ERROR_QUANTILE", raising=False)
            else:
                mp.setenv("EBCC_INIT_BASE_ERROR_QUANTILE", c["quantile"])
            cfg = L.make_config((1, h, w), base_cr=c["base_cr"], error=c["error"], residual_type=c["mode"])
            batches = [[n] for n in names] if i % 2 == 0 else [names]
            for b in batches:
                got = ctx.encode_frames(np.stack([C._inputs[C._streams[n]["input"]] for n in b]), cfg)
                for n, s in zip(b, got):
                    assert s == bytes.fromhex(C._streams[n]["stream_hex"]), (n, len(b))
        mp.delenv("EBCC_INIT_BASE_ERROR_QUANTILE", raising=False)
        hd = ctx.decode_frames(hs)
        names = [n for k in keys for n in sorted(golden[k])]
        for i in range(0, len(names), 4):                       # (a 1-frame batch, then a 3-frame one)
            for b in (names[i:i + 1], names[i + 1:i + 4]):
                dec = ctx.decode_frames([bytes.fromhex(C._streams[n]["stream_hex"]) for n in b])
                for n, d in zip(b, dec):
                    assert sha(d.tobytes()) == C._streams[n]["decoded_sha256"], (n, len(b))
    want = L.orc_encode_many(hostile, hcfg)
    for f, s in enumerate(hs):
        assert s == want[f], f"hostile frame {f}"
        assert S.same_bits(hd[f].ravel(), L.orc_decode(s)), f"hostile decode {f}"


def test_sliced_unsliced_sliced_on_one_context(_clean_env):
    """H2: one 64 x 96 context of 128 frames: 128 frames (sliced), 3 (one slice), 100 with other content (sliced).
    Streams are the oracle's, decoded fields the oracle's decode, and the bound holds in float64 (without the mean
    adjustment, which may move the error past the bound - the reference does that too)."""
    _clean_env.setenv("EBCC_DISABLE_MEAN_ADJUSTMENT", "1")      # (the oracle's spawned workers inherit it)
    lib = L.product()
    lib.ebcc_hip_encode_slices_for.argtypes = [ctypes.c_size_t]
    lib.ebcc_hip_encode_slices_for.restype = ctypes.c_int
    assert lib.ebcc_hip_encode_slices_for(128) > 1 and lib.ebcc_hip_encode_slices_for(3) == 1
    h, w, err = 64, 96, 0.05
    cfg = L.make_config((1, h, w), base_cr=20.0, error=err, residual_type=L.MAX_ERROR)
    runs = [np.stack([L.era5_like(h, w, s, 1.0 + 0.1 * (s % 7), 0.5 + 0.3 * (s % 4)) for s in range(128)]),
            np.stack([L.era5_like(h, w, 900 + s, 1.3, 3.0) for s in range(3)]),
            np.stack([L.era5_like(h, w, 1000 + s, 1.6, 2.0 + (s % 3)) for s in range(100)])]
    with L.Context(128, h, w) as ctx:
        got = [ctx.encode_frames(x, cfg) for x in runs]
        dec = [ctx.decode_frames(g) for g in got]
    for r, (x, g, d) in enumerate(zip(runs, got, dec)):
        want = L.orc_encode_many(x, cfg)
        for f in range(len(x)):
            assert g[f] == want[f], (r, f)
            assert S.same_bits(d[f].ravel(), L.orc_decode(g[f])), (r, f)
            assert np.abs(d[f].astype(np.float64) - x[f].astype(np.float64)).max() <= float(np.float32(err)), (r, f)


def test_engines_made_again_by_the_public_api(_clean_env):
    """H3: ebcc_encode_chunking / ebcc_decode_chunking on one geometry with 2, 40 and 3 chunks (the engines are made
    again, larger, in between), then ebcc_hip_release_engines, another shape, and the first again: every container and
    every decode is the oracle's."""
    lib = L.product()
    lib.ebcc_hip_release_engines.restype = None
    L.oracle().orc_set_j2k_backend(0)

    def run(n, h, w, seed):
        x = np.stack([L.era5_like(h, w, seed + s, 1.1 + 0.1 * (s % 4), 0.6 + 0.4 * (s % 3)) for s in range(n)])
        cfg = L.make_config(x.shape, (1, h, w), base_cr=20.0, error=0.05, residual_type=L.MAX_ERROR)
        s = C.api_encode(x, cfg, "ebcc_encode_chunking")
        want = L.orc_encode(x, cfg, "orc_ebcc_encode_chunking")
        assert s == want, (n, h, w)
        assert S.same_bits(C.api_decode(s, "ebcc_decode_chunking"), L.orc_decode(want, "orc_ebcc_decode_chunking")), (n, h, w)

    run(2, 64, 96, 300)
    run(40, 64, 96, 400)
    run(3, 64, 96, 500)
    lib.ebcc_hip_release_engines()
    run(4, 100, 130, 600)
    run(3, 64, 96, 700)
    run(2, 64, 96, 300)
