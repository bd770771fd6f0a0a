"""GPU: the probes of the rate search against real encodes and decodes of the CPU oracle, over sequences of rates.

A round of the search (launch_j2k_rate + launch_j2k_probe_decode) reports count(|x - d| > target), sum(x - d) and the
codestream's length at a rate, restarting the tier-1 decode from the encoder's checkpoints; what jb.V, the layer assignment
and the checkpoints hold carries over from probe to probe.  ebcc_hip_j2k_probe runs such a round through the search's own
launchers; here it walks rate sequences on ONE tier-1 encoding, and after every probe the statistics, the length and - where
the probe stores it - the field are compared with a fresh encode + decode of the oracle at that rate (tests/_probes.py).
The early count (J2kFrame::bad_limit) is held to its contract (search.hpp)."""
import functools

import numpy as np
import pytest

from tests import _fields as F
from tests import _lib as L
from tests import _probes as P
from tests.test_j2k_gpu import _fields

pytestmark = pytest.mark.gpu

GEOMS = [(32, 32), (33, 47), (100, 130), (181, 360), (37, 2047), (2047, 33)]
WALKS = {"search": [30, 15, 7.5, 3.75, 5.6, 4.7],                      # halve, then bisect
         "hostile": [30, 1000, 1, 1000, 2, 1.5, 500, 30, 30]}           # the largest jumps both ways, a rate twice
TARGETS = ["p50", "p99", "max"]
KEEP_MODES = [1, 0, 2, 2, 0, 1, 2, 0, 1]                                 # keep_field of step i (the first one stores every field)
COUNT = {"frame-rate-target-limit": 0}


@functools.lru_cache(maxsize=None)
def fields(h, w):
    return np.ascontiguousarray(np.concatenate([_fields(h, w), np.stack([F.field(k, h, w) for k in ("noise", "spike", "checker")])]))


@functools.lru_cache(maxsize=None)
def at_rate(h, w, f, cr):
    """(d, length, e = x - d, |e| sorted) of field f at rate cr"""
    x = fields(h, w)[f]
    d, n = P.base_layer(x, cr)
    e = P.rate_errors(x, d)
    return d, n, e, np.sort(np.abs(e).ravel())


def target_of(h, w, f, cr, which):
    """order statistics of the reference's own |x - d| (sample values: the comparison is strict); the maximum counts 0"""
    a = at_rate(h, w, f, cr)[3]
    return a[{"p50": (a.size - 1) // 2, "p99": ((a.size - 1) * 99) // 100, "max": a.size - 1}[which]]


def check_stats(h, w, f, cr, target, nbad, esum, size, limit=0):
    _, n, e, _ = at_rate(h, w, f, cr)
    COUNT["frame-rate-target-limit"] += 1
    assert int(size) == n, (f, cr, int(size), n)
    want = P.count_bad(e, target)
    if limit and want >= limit:
        assert limit <= int(nbad) <= want, (f, cr, limit, int(nbad), want)
        return
    assert int(nbad) == want, (f, cr, float(target), int(nbad), want)
    assert abs(float(esum) - P.error_sum(e)) <= P.sum_bound(e), (f, cr, float(esum), P.error_sum(e), P.sum_bound(e))


class Rig:
    def __init__(self, h, w, encode_cr=30.0):
        self.h, self.w = h, w
        self.x = fields(h, w)
        self.n = len(self.x)
        self.ctx = L.Context(self.n, h, w)
        streams, mm, self.d = self.ctx.j2k_encode(self.x, [encode_cr] * self.n, keep_device=True)
        for f in range(self.n):
            _, mn, mx = L.scale_u16(self.x[f])
            assert mm[f, 0] == mn and mm[f, 1] == mx
            assert len(streams[f]) == at_rate(h, w, f, float(encode_cr))[1]
        self.held = [None] * self.n                                      # the rate whose field jb.DEC holds, per frame

    def probe(self, cr, targets, keep_field, keep=None, active=None, bad_limit=None):
        """one round; checks the stored fields against what must lie there now and returns the statistics"""
        crs = np.broadcast_to(np.asarray(cr, np.float32), (self.n,))
        act = np.ones(self.n, np.int32) if active is None else np.asarray(active, np.int32)
        kp = np.zeros(self.n, np.int32) if keep is None else np.asarray(keep, np.int32)
        nbad, esum, size, field = self.ctx.j2k_probe(self.d, self.n, crs, targets, bad_limit=bad_limit, keep=kp, active=act,
                                                     keep_field=keep_field, want_field=True)
        for f in range(self.n):
            if act[f] and (keep_field == 1 or (keep_field == 2 and kp[f])):
                self.held[f] = float(crs[f])
            if self.held[f] is not None:                                 # (a probe that stores nothing leaves the last kept field)
                assert np.array_equal(field[f], at_rate(self.h, self.w, f, self.held[f])[0]), (f, float(crs[f]), self.held[f], keep_field)
        return nbad, esum, size

    def close(self):
        self.d.free()
        self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


@pytest.mark.parametrize("which", TARGETS)
@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_rate_walk(geom, walk, which):
    h, w = geom
    with Rig(h, w) as rig:
        for i, cr in enumerate(WALKS[walk]):
            cr = float(cr)
            tg = [target_of(h, w, f, cr, which) for f in range(rig.n)]
            keep = [(f + i) % 2 for f in range(rig.n)]
            nbad, esum, size = rig.probe(cr, tg, KEEP_MODES[i], keep=keep)
            for f in range(rig.n):
                check_stats(h, w, f, cr, tg[f], nbad[f], esum[f], size[f])
                if which == "max":
                    assert int(nbad[f]) == 0


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_one_launch_many_rates_and_inactive_frames(geom):
    h, w = geom
    sent = L.Context.PROBE_SENTINEL
    with Rig(h, w) as rig:
        rig.probe(30.0, [0.0] * rig.n, 1)
        for keep_field, rates in ((1, [2.0, 5.0, 9.0, 20.0, 60.0, 400.0]), (0, [400.0, 1.0, 60.0, 3.0, 12.0, 7.0]),
                                  (2, [7.0, 12.0, 3.0, 60.0, 1.0, 400.0])):
            active = [0 if f % 3 == 2 else 1 for f in range(rig.n)]
            keep = [f % 2 for f in range(rig.n)]
            for which in TARGETS:
                tg = [target_of(h, w, f, rates[f], which) for f in range(rig.n)]
                nbad, esum, size = rig.probe(rates, tg, keep_field, keep=keep, active=active)
                for f in range(rig.n):
                    if active[f]:
                        check_stats(h, w, f, rates[f], tg[f], nbad[f], esum[f], size[f])
                    else:                                                # untouched: sentinels here, the old field above
                        assert nbad[f] == sent[0] and esum[f] == sent[1] and size[f] == sent[2], f
        # every frame again, each at the rate an inactive frame was NOT probed at: nothing of the masked rounds sticks to it
        tg = [target_of(h, w, f, 15.0, "p50") for f in range(rig.n)]
        nbad, esum, size = rig.probe(15.0, tg, 1)
        for f in range(rig.n):
            check_stats(h, w, f, 15.0, tg[f], nbad[f], esum[f], size[f])


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_early_count_contract(geom):
    """J2kFrame::bad_limit = L on statistics-only probes, N the exact count: N < L -> the count is N and the sum the full
    sum; otherwise L <= nbad <= N.  A frame whose field is stored counts everything whatever its limit."""
    h, w = geom
    with Rig(h, w) as rig:
        rig.probe(30.0, [0.0] * rig.n, 1)
        for cr in (15.0, 5.0):
            for which in ("p50", "p99"):
                tg = [target_of(h, w, f, cr, which) for f in range(rig.n)]
                exact = [P.count_bad(at_rate(h, w, f, cr)[2], tg[f]) for f in range(rig.n)]
                for make in (lambda n: 1, lambda n: max(1, n // 2), lambda n: max(1, n), lambda n: n + 1, lambda n: n + 1000):
                    lim = [make(n) for n in exact]
                    for keep_field, keep in ((0, [0] * rig.n), (2, [f % 2 for f in range(rig.n)])):
                        nbad, esum, size = rig.probe(cr, tg, keep_field, keep=keep, bad_limit=lim)
                        for f in range(rig.n):
                            stored = keep_field == 2 and keep[f]
                            check_stats(h, w, f, cr, tg[f], nbad[f], esum[f], size[f], limit=0 if stored else lim[f])


def test_zz_comparisons_made():
    print(f"\nrate probe comparisons (frame, rate, target, limit): {COUNT['frame-rate-target-limit']}")
