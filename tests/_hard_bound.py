"""The hard-bound rule of include/ebcc_hip.h restated on the oracle (CPU; shared by the audit and hard-bound GPU tests and
by tools/gpu/hard_rate.py's reading of them): per frame, encode with the config's error, decode, measure max |x - x^| in
float32, and while it is above the target T re-encode with e' = (e * (T / a)) * 0.9 in float32 - at most `max_rounds`
re-encodes (0 means 6), stopping early when e' is 0 or not below e; a frame that is not met keeps the stream of the round
with the smallest error, the earliest on ties.  Nothing here touches a device."""
import numpy as np

from tests import _lib as L

F32 = np.float32
#       name: (height, width, seeds, mode, error, base_cr, environment)
SETS = {"max_64x96": (64, 96, 16, L.MAX_ERROR, 0.02, 20.0, {}),
        "max_40x50": (40, 50, 12, L.MAX_ERROR, 0.01, 10.0, {}),
        "rel_64x96": (64, 96, 12, L.RELATIVE_ERROR, 0.004, 20.0,
                      {"EBCC_INIT_BASE_ERROR_QUANTILE": "0.02", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK": "1"})}
ENV_NAMES = ("EBCC_INIT_BASE_ERROR_QUANTILE", "EBCC_DISABLE_PURE_BASE_COMPRESSION_FALLBACK")
_made = {}


def once(key, make):
    """a value made once per process and shared by the tests (inputs, oracle streams, oracle loops): never changed"""
    if key not in _made:
        _made[key] = make()
    return _made[key]


def use_env(monkeypatch, env):
    """the encoder's environment switches of a set, for the oracle and the product alike"""
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    L.oracle().orc_set_j2k_backend(0)


def set_inputs(name):
    h, w, n = SETS[name][:3]
    return once(("inputs", h, w, n), lambda: inputs(h, w, range(n)))


def set_loop(name, max_rounds=0):
    """[(stream, report, history)] of the set's frames under the rule (the caller has set the set's environment)"""
    _h, _w, _n, mode, err, cr, _env = SETS[name]
    return once(("loop", name, max_rounds), lambda: [harden(x, mode, err, cr, max_rounds) for x in set_inputs(name)])


def inputs(h, w, seeds):
    a = np.stack([L.era5_like(h, w, s, 1.0 + 0.1 * (s % 4), 0.6 + 0.3 * (s % 3)) for s in seeds])
    a.setflags(write=False)
    return a


def stats(x, d, bound=None):
    """the record ebcc_hip_frame_errors gives for one frame, with numpy: (max_abs, at, n_over, sum, sum_sq, x_min, x_max)"""
    x, d = np.ascontiguousarray(x, F32).ravel(), np.ascontiguousarray(d, F32).ravel()
    ab = np.abs(x - d)                                            # float32 arithmetic
    e = x.astype(np.float64) - d.astype(np.float64)
    at = int(np.argmax(ab))                                      # (first occurrence)
    n_over = int((ab > F32(bound)).sum()) if bound is not None else 0
    return (F32(ab[at]), at, n_over, float(e.sum()), float((e * e).sum()), F32(x.min() + F32(0)), F32(x.max() + F32(0)))


def target(x, mode, error):
    if mode == L.MAX_ERROR:
        return F32(error)
    if mode == L.RELATIVE_ERROR:
        return F32(F32(error) * F32(F32(x.max()) - F32(x.min())))
    return F32(np.inf)


def harden(x, mode, error, base_cr, max_rounds=0, target_value=None):
    """-> (stream, report, history): report = (target, achieved, error_used, rounds, met) as ebcc_hip_bound_report, history =
    [(e_k, a_k, bytes)] of every round.  target_value: the bound restated for a group with range_of_group (mode MAX_ERROR)."""
    h, w = x.shape
    cap = max_rounds if max_rounds > 0 else 6
    T = target(x, mode, error) if target_value is None else F32(target_value)
    e = F32(error)
    if mode == L.NONE:
        s = L.orc_encode(x, L.make_config((1, h, w), base_cr=base_cr, error=0.0, residual_type=mode))
        a = stats(x, L.orc_decode(s))[0]
        return s, (T, a, e, 0, 1), [(e, a, len(s))]
    best, hist, k = None, [], 0
    while True:
        s = L.orc_encode(x, L.make_config((1, h, w), base_cr=base_cr, error=float(e), residual_type=mode))
        assert s
        a = stats(x, L.orc_decode(s))[0]
        hist.append((e, a, len(s)))
        if best is None or a < best[1]:
            best = (s, a, e)
        if a <= T:
            return s, (T, a, e, k, 1), hist
        if k == cap:
            break
        nxt = F32(F32(e * F32(T / a)) * F32(0.9))
        if nxt == 0 or not nxt < e:
            break
        e, k = nxt, k + 1
    return best[0], (T, best[1], best[2], k, 0), hist
