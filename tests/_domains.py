"""Catalogue of deterministic frame-codec cases over value domains, error targets, start rates and base-layer
quantiles, chosen so that between them they take every branch of the two error-bound searches of the reference
(src/ebcc_codec.c:545-596 rate search, :730-854 residual / truncation / fallback) - tests/test_search_branches.py
checks that they still do, tests/golden/search_branches.json holds what the reference build wrote for each.

A case is (name, generator, shape, mode, error, base_cr, quantile).  `error` is the value handed to the codec:
MAX_ERROR cases give it as a fraction of the field's range (converted here, in float64, then stored as f32 by the
config), RELATIVE_ERROR cases give the fraction itself.
"""
import os
import subprocess
import sys

import numpy as np

from tests import _lib as L

SHAPES = [(64, 96), (100, 130), (37, 70)]


def _rng(seed):
    return np.random.default_rng(seed)


def temperature(h, w, seed):
    return L.era5_like(h, w, seed)


def wind(h, w, seed):
    """zonal wind: smooth, about +-30, crosses zero"""
    n = L.era5_like(h, w, seed, amp=1.0) - np.float32(235.0)
    n = (n - n.mean()) / n.std()
    return (12.0 * n).astype(np.float32)


def geopotential(h, w, seed):
    """1e5 + 50 z: the f32 ulp (0.0078) is comparable to tight bounds"""
    z = L.smooth_image(h, w, seed).astype(np.float64) * 2.0 - 1.0
    return (1e5 + 50.0 * z).astype(np.float32)


def humidity(h, w, seed):
    """specific humidity: lognormal around 1e-3"""
    z = L.smooth_image(h, w, seed).astype(np.float64)
    return (1e-3 * np.exp(2.0 * (z - 0.5) + 0.1 * _rng(seed).standard_normal((h, w)))).astype(np.float32)


def tiny(h, w, seed):
    """values about 1e-30 (normal floats, far below 1)"""
    return (L.smooth_image(h, w, seed).astype(np.float64) * 3e-30 + 1e-30).astype(np.float32)


def subnormal(h, w, seed):
    """multiples of the smallest subnormal: any flush of denormals on the device changes the stream"""
    k = np.floor(L.smooth_image(h, w, seed).astype(np.float64) * 200.0)
    return (k * 1.401298464324817e-45).astype(np.float32)


def precipitation(h, w, seed):
    """sparse: exact 0 outside a few rain cells (threshold at the 85th percentile: never a constant field)"""
    z = L.smooth_image(h, w, seed).astype(np.float64)
    t = np.quantile(z, 0.85)
    return np.where(z > t, (z - t) * 40.0, 0.0).astype(np.float32)


def mask(h, w, seed):
    """binary land-sea mask"""
    return (L.smooth_image(h, w, seed) > 0.5).astype(np.float32)


def noise(h, w, seed):
    """white noise in [0, 1)"""
    return _rng(seed).random((h, w)).astype(np.float32)


def narrow(h, w, seed):
    """values a few ulps apart around 1000: the u16 scaling uses a handful of levels"""
    k = np.floor(L.smooth_image(h, w, seed) * 6.0).astype(np.int32)
    return np.nextafter(np.float32(1000.0), np.float32(np.inf)) + k.astype(np.float32) * np.float32(6.103515625e-05)


def signed_zeros(h, w, seed):
    """+0.0 and -0.0 mixed with a few non-zero values"""
    r = _rng(seed)
    a = np.where(r.random((h, w)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    idx = r.choice(h * w, 5, replace=False)
    a.flat[idx] = np.array([1.5, -2.0, 0.25, 3.0, -0.5], np.float32)
    return a


def large(h, w, seed):
    """about +-1e38 with a finite range (max - min below FLT_MAX)"""
    z = L.smooth_image(h, w, seed).astype(np.float64) * 2.0 - 1.0
    return (1.5e38 * z).astype(np.float32)


def overflow(h, w, seed):
    """about +-3e38: max - min overflows to inf in f32"""
    z = L.smooth_image(h, w, seed).astype(np.float64) * 2.0 - 1.0
    return (3e38 * z).astype(np.float32)


def constant(h, w, seed):
    return np.full((h, w), 273.15, np.float32)


DOMAINS = {f.__name__: f for f in (temperature, wind, geopotential, humidity, tiny, subnormal, precipitation, mask, noise,
                                   narrow, signed_zeros, large, overflow, constant)}


ERRORS = [(L.MAX_ERROR, 0.6), (L.MAX_ERROR, 1e-2), (L.MAX_ERROR, 2e-3), (L.MAX_ERROR, 1e-6),
          (L.RELATIVE_ERROR, 0.3), (L.RELATIVE_ERROR, 1e-4), (L.RELATIVE_ERROR, 1e-7)]
BASE_CRS = [0.75, 1.0, 30.0, 1000.0, 2000.0]
QUANTILES = [None, "0.02", "0.1"]         # EBCC_INIT_BASE_ERROR_QUANTILE (None: unset, the reference's 1e-6)
_GRID_DOMAINS = ["temperature", "wind", "geopotential", "humidity", "tiny", "subnormal", "precipitation", "mask", "noise",
                 "narrow", "signed_zeros", "large"]


class Case:
    def __init__(self, domain, shape, mode, frac, base_cr, quantile, seed=1):
        self.domain, self.shape, self.mode, self.frac, self.base_cr, self.quantile, self.seed = \
            domain, tuple(shape), mode, frac, base_cr, quantile, seed
        m = {L.NONE: "none", L.MAX_ERROR: "abs", L.RELATIVE_ERROR: "rel"}[mode]
        self.name = f"{domain}-{shape[0]}x{shape[1]}-{m}{frac:g}-cr{base_cr:g}-q{quantile or 'default'}"

    def field(self):
        return DOMAINS[self.domain](*self.shape, self.seed)

    def config(self, field=None):
        x = self.field() if field is None else field
        err = self.frac
        if self.mode == L.MAX_ERROR:                       # a fraction of the range, worked out in float64
            err = self.frac * (float(np.float64(x.max())) - float(np.float64(x.min())))
        return L.make_config((1,) + self.shape, base_cr=self.base_cr, error=err, residual_type=self.mode)

    def target(self, field=None):
        """The error target the codec works with (:723-726), in float32 as it does - 0 for a bound that underflows."""
        x = self.field() if field is None else field
        t = np.float32(self.config(x).error)
        if self.mode == L.RELATIVE_ERROR:
            t = np.float32(t * (np.float32(x.max()) - np.float32(x.min())))
        return t

    def bound64(self, field=None):
        """The same bound in float64: the target, or relative x range."""
        x = self.field() if field is None else field
        if self.mode == L.RELATIVE_ERROR:
            return float(np.float32(self.frac)) * (float(np.float64(x.max())) - float(np.float64(x.min())))
        return float(np.float32(self.config(x).error))


def catalogue():
    """Every domain against every error target once, start rate, quantile and shape rotating with it (each domain sees
    five start rates, all three quantiles and all three shapes), plus the cases that reach what the grid does not.
    Cases whose target underflows to 0 in float32 are left out: the reference asserts error_target > 0 (:826)."""
    cases = []
    for i, d in enumerate(_GRID_DOMAINS):
        for j, (mode, frac) in enumerate(ERRORS):
            cases.append(Case(d, SHAPES[(i + j) % 3], mode, frac, BASE_CRS[(i + j) % 5], QUANTILES[(i + 2 * j) % 3]))
    cases += [
        Case("constant", (64, 96), L.MAX_ERROR, 0.01, 30.0, None),
        Case("constant", (37, 70), L.RELATIVE_ERROR, 1e-4, 2000.0, "0.1"),
        Case("temperature", (64, 96), L.NONE, 0.0, 30.0, None),
    ]
    return [c for c in cases if c.mode == L.NONE or c.domain == "constant" or c.target() > 0]


def overflow_case():
    """max - min overflows float32 (values at +-3e38).  See tests/test_search_branches.py for what the reference does."""
    return Case("overflow", (64, 96), L.MAX_ERROR, 1e-2, 30.0, None)


_REF_CHILD = """
import sys
sys.path.insert(0, {root!r})
from tests import _domains as D, _lib as L
c = [c for c in D.catalogue() + [D.overflow_case()] if c.name == {name!r}][0]
s = L.ref_encode(c.field(), c.config())
print(len(s))
"""


def reference_refuses(case):
    """Run the reference build's ebcc_encode on `case` in a child process: True if it wrote no stream (returned 0, or
    stopped - the reference asserts and exits on some inputs)."""
    env = {k: v for k, v in os.environ.items() if k != "EBCC_INIT_BASE_ERROR_QUANTILE"}
    if case.quantile is not None:
        env["EBCC_INIT_BASE_ERROR_QUANTILE"] = case.quantile
    r = subprocess.run([sys.executable, "-c", _REF_CHILD.format(root=L.ROOT, name=case.name)], capture_output=True,
                       text=True, env=env, timeout=300)
    return r.returncode != 0 or r.stdout.strip() == "0"
