"""GPU: the probes of the truncation search against real decodes of the CPU oracle, densely over the cuts.

A probe (launch_prefix_synthesis_stats, and its look-ahead form launch_prefix_synthesis_slots) reports max |x - (d + r')| and
sum(x - (d + r')) for a cut of the SPIHT stream without decoding anything: it rebuilds the decoder's state from the
encoder's bookkeeping.  The whole-codec tests see these numbers only where they flip a comparison of the bisection; here every
one of them is compared with tests/_probes.py (pinned to the oracle by tests/test_probe_reference.py) through
ebcc_hip_residual_prepare / ebcc_hip_residual_probe, which call the encoder's own launchers.

Geometries: where the strips of 60 pairs, the pieces (min(8, (ny / 2) / 16)), the crop and the 8-byte loads change.
Inputs: a smooth field against its real base layer, and designed residuals - full-range noise, the 0/1 checkerboard, a small
smooth residual with one dominating spike at the places a wrong crop mask or boundary tap would lose it.
Cuts: every byte for the three smallest geometries; first 256, last 64, a 3 % ladder and the cuts the restated bisection
visits for the rest.  The per-cut maximum is not monotone in the cut; nothing here assumes it is."""
import functools

import numpy as np
import pytest

from tests import _fields as F
from tests import _lib as L
from tests import _probes as P

pytestmark = pytest.mark.gpu

GEOMS = [(32, 32), (33, 47), (64, 130), (100, 130), (264, 250), (40, 2047), (2047, 40)]
DENSE = GEOMS[:3]
COUNT = {"frame-cut": 0}


def _pieces(h):
    ny = h + (-h) % 16
    half = ny // 2
    pieces = max(1, min(8, half // 16))
    return pieces, -(-half // pieces)


def spike_places(h, w):
    """name -> (row, col): the corners, the middle of the last row and of the last column, the columns around the edge of
    the first strip (pair 60 = column 120), the first and the last row of the second piece"""
    at = {"tl": (0, 0), "tr": (0, w - 1), "bl": (h - 1, 0), "br": (h - 1, w - 1), "bottom": (h - 1, w // 2),
          "right": (h // 2, w - 1)}
    for c in (119, 120, 121):
        if c < w:
            at[f"col{c}"] = (h // 2, c)
    pieces, per = _pieces(h)
    if pieces > 1 and 2 * per < h:
        at["piece1-first"] = (2 * per, w // 3)
        at["piece1-last"] = (min(4 * per - 1, h - 1), w // 3)
    return at


def input_names(h, w):
    return ["base", "noise", "checker"] + [f"spike-{k}" for k in spike_places(h, w)]


def designed_budget(h, w):
    """the SPIHT budget in bits of the designed residuals (also tests/test_geometry_sweep_gpu.py)"""
    return 8 * min(1600, max(200, (h * w) // 5))


@functools.lru_cache(maxsize=None)
def make_input(h, w, name):
    """(x, d, budget in bits)"""
    x = L.era5_like(h, w, 3 * h + w)
    if name == "base":
        d, nbytes = P.base_layer(x, 60.0)
        return x, d, 8 * min(nbytes, 1600)
    if name == "noise":
        r = F.noise(h, w, 1)
    elif name == "checker":
        r = F.checker(h, w, 0)
    else:
        r = (L.smooth_image(h, w, 5) * np.float32(0.01)).astype(np.float32)
        r[spike_places(h, w)[name[len("spike-"):]]] = 1.0
    d = (x - r).astype(np.float32)
    return x, d, designed_budget(h, w)


@functools.lru_cache(maxsize=None)
def reference(h, w, name):
    """the residual layer of the input, its cut list (bytes) and the two early-exit targets"""
    x, d, budget = make_input(h, w, name)
    res = P.Residual(x, d, budget)
    n = len(res.stream)
    cuts = list(range(17, n + 3)) if (h, w) in DENSE else P.ladder(n)
    maxima = np.array([res.maxerr(c) for c in cuts], np.float32)
    targets = [np.float32(np.median(maxima)), np.float32(maxima[len(maxima) // 3])]     # the median; one cut's maximum exactly
    if (h, w) not in DENSE:
        extra = set()
        for t in targets:
            if res.maxerr(n) <= t:                                       # (:755: the bisection runs on a feasible stream)
                extra |= set(P.bisection(res.maxerr, n, t)[0])
        cuts = sorted(set(cuts) | extra)
    return res, cuts, targets


class Rig:
    """a context with the inputs uploaded and the residual layer prepared"""

    def __init__(self, h, w, names, offset_bytes=0):
        self.h, self.w, self.names = h, w, list(names)
        n = self.n = len(self.names)
        xs = np.stack([make_input(h, w, k)[0] for k in self.names])
        ds = np.stack([make_input(h, w, k)[1] for k in self.names])
        self.ctx = L.Context(n, h, w)
        self.bx, self.bd = L.DeviceArray(nbytes=xs.nbytes + 16), L.DeviceArray(nbytes=ds.nbytes + 16)
        self.x, self.d = self.bx.ptr + offset_bytes, self.bd.ptr + offset_bytes
        lib = L.product()
        assert lib.ebcc_hip_memcpy_h2d(self.x, xs.ctypes.data, xs.nbytes) == 0
        assert lib.ebcc_hip_memcpy_h2d(self.d, ds.ctypes.data, ds.nbytes) == 0
        self.prep = self.ctx.residual_prepare(self.x, self.d, n, [make_input(h, w, k)[2] for k in self.names])

    def frames(self, cut_bytes, **kw):
        return self.ctx.residual_probe(self.x, self.d, self.n, list(range(self.n)), [8 * c for c in cut_bytes], **kw)

    def slots(self, frame_of, cut_bytes, chunk=2048, **kw):
        bits, sums = [], []
        for i in range(0, len(cut_bytes), chunk):
            sub = {k: (v[i:i + chunk] if np.ndim(v) else v) for k, v in kw.items()}
            b, s = self.ctx.residual_probe(self.x, self.d, self.n, frame_of[i:i + chunk], [8 * c for c in cut_bytes[i:i + chunk]],
                                           slots=True, **sub)
            bits.append(b)
            sums.append(s)
        return np.concatenate(bits), np.concatenate(sums)

    def close(self):
        self.ctx.close()
        self.bx.free()
        self.bd.free()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def check_prepared(rig):
    """the residual layer the probes rest on is the reference's: range, and the SPIHT stream byte for byte"""
    rmin, rmax, _dc, streams = rig.prep
    for f, name in enumerate(rig.names):
        res = reference(rig.h, rig.w, name)[0]
        assert P.f32_bits(rmin[f]) == P.f32_bits(res.rmin) and P.f32_bits(rmax[f]) == P.f32_bits(res.rmax), name
        assert streams[f] == res.stream, name


def check_exact(res, cuts, bits, sums, what):
    bad = []
    for c, b, s in zip(cuts, bits, sums):
        wb, ws, bound = res.stats(c)
        COUNT["frame-cut"] += 1
        if int(b) != wb or not abs(float(s) - ws) <= bound:
            bad.append((c, hex(int(b)), hex(wb), float(s), ws, bound))
    assert not bad, (what, len(bad), bad[:8])


CASES = [pytest.param((h, w, k), id=f"{h}x{w}-{k}") for h, w in GEOMS for k in input_names(h, w)]


@pytest.mark.parametrize("case", CASES)
def test_exact_probes_equal_real_decodes(case):
    h, w, name = case
    res, cuts, _ = reference(h, w, name)
    with Rig(h, w, [name]) as rig:
        check_prepared(rig)
        one = [rig.frames([c]) for c in cuts]                           # the one-cut-per-round form, a cut a launch
        check_exact(res, cuts, [b[0] for b, _ in one], [s[0] for _, s in one], "frames")
        bits, sums = rig.slots([0] * len(cuts), cuts)                    # the look-ahead form, every cut a slot
        check_exact(res, cuts, bits, sums, "slots")
        # the two forms take their partial sums in the same order
        assert np.array_equal(bits, [b[0] for b, _ in one]) and np.array_equal(sums, [s[0] for _, s in one])


@pytest.mark.parametrize("case", CASES)
def test_early_exit_contract(case):
    """FrameState::exit_above = T: a cut whose maximum is <= T (== T included) comes back as the exact probe, sum and all;
    one above T comes back with T < m <= its maximum, sum unspecified"""
    h, w, name = case
    res, cuts, targets = reference(h, w, name)
    sub = cuts if len(cuts) <= 400 else cuts[::4]                        # (frames form: a launch a cut)
    with Rig(h, w, [name]) as rig:
        exact_b, exact_s = rig.slots([0] * len(cuts), cuts)
        exact = {c: (int(b), float(s)) for c, b, s in zip(cuts, exact_b, exact_s)}
        for t in targets:
            assert any(res.maxerr(c) == t for c in cuts) or t == targets[0]
            got = dict(zip(cuts, zip(*rig.slots([0] * len(cuts), cuts, exit_above=float(t)))))
            got_frames = {c: tuple(v[0] for v in rig.frames([c], exit_above=float(t))) for c in sub}
            for form, g in (("slots", got), ("frames", got_frames)):
                for c, (b, s) in g.items():
                    true = res.maxerr(c)
                    COUNT["frame-cut"] += 1
                    if true <= t:
                        assert (int(b), float(s)) == exact[c], (form, c, t)
                        assert int(b) == res.stats(c)[0], (form, c, t)
                    else:
                        m = P.bits_f32(b)
                        assert t < m <= true, (form, c, float(t), float(m), float(true))


def test_exit_at_the_target_itself_is_exact():
    """exit_above equal to the cut's maximum, which the first wave of the frame finds (a spike in the top left corner), in a
    launch of far more waves than the chip holds at once (2048 slots of 24 strips-by-pieces): the waves that start after the
    maximum is on record must still run - the maximum does not EXCEED the target - and every slot's sum must be whole"""
    h, w, name = 264, 250, "spike-tl"
    res, cuts, targets = reference(h, w, name)
    t = targets[1]
    c = next(c for c in cuts if res.maxerr(c) == t)
    with Rig(h, w, [name]) as rig:
        eb, es = rig.slots([0], [c])
        assert int(eb[0]) == P.f32_bits(t) == res.stats(c)[0]
        bits, sums = rig.slots([0] * 2048, [c] * 2048, exit_above=float(t))
        COUNT["frame-cut"] += 2048
        assert np.all(bits == eb[0]) and np.all(sums == es[0]), (int((bits != eb[0]).sum()), int((sums != es[0]).sum()))


FORM_GEOMS = [(33, 47), (64, 130), (264, 250), (2047, 40)]


@pytest.mark.parametrize("geom", FORM_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_forms_agree(geom):
    """3 and 7 slots a frame, the slots of the frames interleaved, inactive slots, the same cut twice, and the frames form
    under masks that leave frames out: the same bits everywhere, sentinels where nothing was asked"""
    h, w = geom
    names = ["base", "noise", "checker", "spike-br"]
    nf = len(names)
    refs = [reference(h, w, k) for k in names]
    sent_b, sent_s = L.Context.RESID_SENTINEL
    with Rig(h, w, names) as rig:
        check_prepared(rig)
        for per_frame in (3, 7):
            frame_of, cuts = [], []
            for j in range(per_frame):                                   # slot v = j * nf + f: frames interleaved
                for f in range(nf):
                    own = refs[f][1]
                    k = (j * 37 + f * 11) % len(own)
                    frame_of.append(f)
                    cuts.append(own[k] if j != 1 else own[len(own) // 2])
            for f in range(nf):                                          # slot per_frame - 1 of a frame repeats its slot 1
                cuts[(per_frame - 1) * nf + f] = cuts[nf + f]
            active = np.array([0 if v % 5 == 2 else 1 for v in range(len(cuts))], np.int32)
            bits, sums = rig.slots(frame_of, cuts, active=active)
            want = {}
            for j in range(per_frame):
                row = [cuts[j * nf + f] for f in range(nf)]
                for mask in ([1, 0, 1, 0], [0, 1, 0, 1]):                # frames form, half of the frames a launch
                    b, s = rig.frames(row, active=mask)
                    for f in range(nf):
                        if mask[f]:
                            want[j * nf + f] = (int(b[f]), float(s[f]))
                        else:
                            assert b[f] == sent_b and s[f] == sent_s, (j, f)
            for v in range(len(cuts)):
                if not active[v]:
                    assert bits[v] == sent_b and sums[v] == sent_s, v
                    continue
                assert (int(bits[v]), float(sums[v])) == want[v], (per_frame, v)
                wb, ws, bound = refs[frame_of[v]][0].stats(cuts[v])
                COUNT["frame-cut"] += 2
                assert int(bits[v]) == wb and abs(float(sums[v]) - ws) <= bound, (per_frame, v)
            for f in range(nf):
                assert bits[nf + f] == bits[(per_frame - 1) * nf + f] or not (active[nf + f] and active[(per_frame - 1) * nf + f])


def test_misaligned_frames_take_the_scalar_loads():
    """data and decoded 4 bytes off an 8-byte boundary: the 8-byte loads of an even-width frame turn off, the bits stay"""
    h, w, name = 64, 130, "noise"
    res, cuts, _ = reference(h, w, name)
    cuts = cuts[::16] + cuts[-3:]
    with Rig(h, w, [name], offset_bytes=4) as rig:
        assert rig.x % 8 == 4 and rig.d % 8 == 4
        check_prepared(rig)
        one = [rig.frames([c]) for c in cuts]
        check_exact(res, cuts, [b[0] for b, _ in one], [s[0] for _, s in one], "frames")
        check_exact(res, cuts, *rig.slots([0] * len(cuts), cuts), "slots")


@pytest.mark.parametrize("geom", [(64, 130), (264, 250)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_real_decoder_gives_the_same_statistics(geom):
    """ebcc_hip_spiht_decode of the prefix S[:c] - what a reader runs - turned into statistics here: the reference's"""
    h, w = geom
    name = "base"
    res, _, _ = reference(h, w, name)
    cuts = P.ladder(len(res.stream))
    bad = []
    with L.Context(64, h, w) as ctx:
        for i in range(0, len(cuts), 64):
            part = cuts[i:i + 64]
            imgs = ctx.spiht_decode([res.stream[:c] for c in part], [8 * c for c in part])
            for c, rn in zip(part, imgs):
                rr = (rn * res.rng + res.rmin).astype(np.float32)
                e = (res.x - (res.d + rr).astype(np.float32)).astype(np.float32)
                wb, ws, _ = res.stats(c)
                COUNT["frame-cut"] += 1
                if P.f32_bits(np.abs(e).max()) != wb or P.error_sum(e) != ws:
                    bad.append(c)
    assert not bad, bad[:10]


def test_short_cuts_are_refused():
    h, w, name = 32, 32, "noise"
    with Rig(h, w, [name]) as rig:
        for slots in (False, True):
            assert rig.ctx.residual_probe(rig.x, rig.d, 1, [0], [128], slots=slots, rc_only=True) == 1
            assert rig.ctx.residual_probe(rig.x, rig.d, 1, [0], [136], slots=slots, rc_only=True) == 0
        assert rig.ctx.residual_probe(rig.x, rig.d, 1, [1], [800], slots=True, rc_only=True) == 1       # no such frame


def test_zz_comparisons_made():
    print(f"\nresidual probe comparisons (frame, cut): {COUNT['frame-cut']}")
