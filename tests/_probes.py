"""Reference of the probes of the two error-bound searches: plain numpy float32 and the CPU oracle, nothing of the product.

Rate probe (src/ebcc_codec.c:545-596, one step): the base layer coded at a rate, really decoded, and the statistics the
search reads of that decode (:494-513).  Truncation probe (:745-754, :777-795, one step): the residual r = x - d normalised,
SPIHT-coded with a budget, a prefix of the stream really decoded, and max |x - (d + r')|, sum(x - (d + r')) (:477-501).
tests/test_probe_reference.py pins both, and the restated bisection, to the oracle's whole encode.
"""
import ctypes
import math
import struct

import numpy as np

from tests import _lib as L

F32 = np.float32


def f32_bits(v):
    return int(np.asarray(v, F32).view(np.uint32))


def bits_f32(b):
    return np.asarray(b, np.uint32).view(F32)


def sum_bound(e):
    """|s - fsum(e)| for a double sum s of the float32 terms e taken in any order: n - 1 additions, each off by at most
    2^-53 of a partial sum no larger than sum |e_i| (1 + 2^-53)^n - below n 2^-52 sum |e_i| for every n here."""
    e = np.asarray(e, np.float64)
    return e.size * 2.0 ** -52 * float(np.abs(e).sum())


def error_sum(e):
    return math.fsum(np.asarray(e, F32).astype(np.float64).ravel().tolist())


# ------------------------------------------------------------------------------------------ rate probe
def base_layer(x, cr):
    """(d, len(s)): the field j2k_decode_internal returns for the codestream j2k_encode_internal writes at rate cr"""
    u16, mn, mx = L.scale_u16(x)
    s = L.orc_j2k_encode(u16, float(cr))
    return L.map_decoded(L.orc_j2k_decode(s), mn, mx), len(s)


def rate_errors(x, d):
    """the float32 differences x - d"""
    return (np.asarray(x, F32) - np.asarray(d, F32)).astype(F32)


def count_bad(e, target):
    return int((np.abs(e) > F32(target)).sum())


# ------------------------------------------------------------------------------------------ truncation probe
class Residual:
    """The residual layer of (x, d) with a SPIHT budget of budget_bits, as :730-748 make it."""

    def __init__(self, x, d, budget_bits):
        self.x = np.ascontiguousarray(x, F32)
        self.d = np.ascontiguousarray(d, F32)
        self.h, self.w = self.x.shape
        r = (self.x - self.d).astype(F32)
        self.rmin, self.rmax = F32(r.min()), F32(r.max())                  # findMinMaxf
        self.rng = F32(self.rmax - self.rmin)
        rn = ((r - self.rmin) / self.rng).astype(F32)                      # :745
        self.budget_bits = int(budget_bits)
        self.stream = L.orc_spiht_encode(rn, self.budget_bits)             # :747-748
        self._cache = {}

    def errors(self, c):
        """e = x - (d + r') for the cut of c bytes, float32 throughout (:779-783); a cut beyond the stream is the
        decoder's clamp of num_bits to the header's bit count (zero bytes stand where the reference would read on)"""
        s = self.stream[:c] if c <= len(self.stream) else self.stream + bytes(c - len(self.stream))
        rn = L.orc_spiht_decode(s, self.h, self.w, 8 * c)
        rr = (rn * self.rng + self.rmin).astype(F32)
        return (self.x - (self.d + rr).astype(F32)).astype(F32)

    def stats(self, c):
        """(float bits of max |e|, fsum(e), bound of a double sum of e) of the cut of c bytes"""
        if c not in self._cache:
            e = self.errors(c)
            self._cache[c] = (f32_bits(np.abs(e).max()), error_sum(e), sum_bound(e))
        return self._cache[c]

    def maxerr(self, c):
        return bits_f32(self.stats(c)[0])


def bisection(maxerr, n_bytes, target):
    """:766-796 over the per-cut maxima maxerr(c bytes) of a stream of n_bytes whose whole decode is feasible:
    (cuts visited in order, in bytes; coeffs_size)"""
    target = F32(target)
    best_err = F32(maxerr(n_bytes))                                       # :754, :761
    assert best_err <= target
    hi, lo = float(n_bytes) * 8, 112.0
    best = hi
    visited = []
    while float(F32(F32(target - best_err) / target)) > 1e-8 and hi - lo > 8 * 4:          # :777
        bits = int(math.ceil((hi + lo) / 2 / 8)) * 8                                       # :778
        cur = F32(maxerr(bits // 8))
        visited.append(bits // 8)
        if cur > target:
            lo = float(bits)
        else:
            hi = float(bits)
            if cur >= best_err:
                best_err, best = cur, float(bits)
    return visited, int(best / 8.0)


def ladder(n_bytes, first=256, last=64, step=1.03):
    """every byte of the first `first` and the last `last` cuts of 17 .. n_bytes, a geometric ladder between them"""
    cuts = set(range(17, min(17 + first, n_bytes + 1))) | set(range(max(17, n_bytes - last + 1), n_bytes + 1))
    c = float(17 + first)
    while c < n_bytes - last:
        cuts.add(int(c))
        c *= step
    return sorted(cuts)


# ------------------------------------------------------------------------------------------ the oracle's stream
def _zstd():
    for name in ("/opt/conda/lib/libzstd.so.1", "libzstd.so.1", "libzstd.so"):
        try:
            z = ctypes.CDLL(name)
        except OSError:
            continue
        z.ZSTD_decompress.restype = ctypes.c_size_t
        z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        return z
    raise OSError("no libzstd (the oracle loads the same one)")


def frame_stream_parts(stream):
    """(rmin, rmax, SPIHT prefix) of a frame stream (header of 48 bytes, zstd payload, codestream)"""
    magic, ver, _flags, _r, _mn, _mx, coeffs, rmn, rmx, zsize, tsize = struct.unpack("<4sBBHIIQIIQQ", stream[:48])
    assert magic == b"EBCC" and ver == 1 and len(stream) == 48 + zsize + tsize
    out = ctypes.create_string_buffer(max(1, coeffs))
    n = _zstd().ZSTD_decompress(out, coeffs, stream[48:48 + zsize], zsize) if zsize else 0
    assert n == coeffs
    return bits_f32(rmn), bits_f32(rmx), out.raw[:coeffs]
