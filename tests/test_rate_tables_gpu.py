"""Rate allocation from the per-code-block walk tables (ebcc_amd/csrc/rate_walk.hpp, k_rate_tables, k_rate) against the
same allocation walking the pass tables at every threshold (EBCC_HIP_RATE_WALK=1) and against the oracle: bytes only.

The switch is read when a context is made, so every comparison makes its contexts under the environment it wants."""
import numpy as np
import pytest

from tests import _lib as L
from tests.test_j2k_gpu import RATES, _fields

pytestmark = pytest.mark.gpu

# the six rates of the ladder and twenty between 2 and 200
LADDER = RATES + [float(np.float32(r)) for r in np.geomspace(2.0, 200.0, 20)]
SWITCHES = ("EBCC_HIP_RATE_WALK", "EBCC_HIP_SPECULATION")


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _ladder_run(fields, rates, monkeypatch, env):
    """streams of every field at every rate (a fresh analysis per call: the first, cold call of a frame), then the same rates
    as probes of one analysis (the later calls of a frame: replayed steps, computed steps, the tail)"""
    _env(monkeypatch, env)
    n, (h, w) = len(fields), fields.shape[1:]
    with L.Context(n, h, w) as ctx:
        streams = [ctx.j2k_encode(fields, [cr] * n)[0] for cr in rates]
        _, _, d = ctx.j2k_encode(fields, [rates[0]] * n, keep_device=True)
        probes = []
        for cr in rates + rates[::-1]:
            nbad, esum, size, _ = ctx.j2k_probe(d, n, cr, 0.25)
            probes.append((nbad.tolist(), esum.tolist(), size.tolist()))
        d.free()
    return streams, probes


@pytest.mark.parametrize("shape", [(33, 47), (100, 130), (181, 360)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_table_mode_equals_walk_mode_and_the_oracle(shape, monkeypatch):
    fields = _fields(*shape)
    tab, tab_probes = _ladder_run(fields, LADDER, monkeypatch, {})
    walk, walk_probes = _ladder_run(fields, LADDER, monkeypatch, {"EBCC_HIP_RATE_WALK": "1"})
    assert tab_probes == walk_probes
    u16 = [L.scale_u16(f)[0] for f in fields]
    for i, cr in enumerate(LADDER):
        for f in range(len(fields)):
            ref = L.orc_j2k_encode(u16[f], cr)
            assert tab[i][f] == ref, ("table", cr, f)
            assert walk[i][f] == ref, ("walk", cr, f)
            # the probes of one analysis, up the ladder and down again: the stream a probe's layer would make
            assert tab_probes[i][2][f] == len(ref) and tab_probes[2 * len(LADDER) - 1 - i][2][f] == len(ref), (cr, f)


def test_more_code_blocks_than_threads(monkeypatch):
    """1536 x 1536: about 580 code-blocks for k_rate's 512 threads, and pass tables that never fitted in LDS"""
    fields = _fields(1536, 1536)[:2]
    rates = [3.0, 30.0, 120.0]
    tab, tab_probes = _ladder_run(fields, rates, monkeypatch, {})
    walk, walk_probes = _ladder_run(fields, rates, monkeypatch, {"EBCC_HIP_RATE_WALK": "1"})
    assert tab == walk
    assert tab_probes == walk_probes
    assert len({len(s[0]) for s in tab}) == len(rates)                 # (the rates did ask for different layers)


@pytest.mark.parametrize("mode,err", [(L.MAX_ERROR, 0.5), (L.RELATIVE_ERROR, 1e-3)], ids=["max_error", "relative_error"])
@pytest.mark.parametrize("shape,n", [((181, 360), 4), ((721, 1440), 2)], ids=["181x360", "721x1440"])
def test_whole_encode(shape, n, mode, err, monkeypatch):
    """both rate searches, the speculative candidates and the final allocation of the pure frames"""
    h, w = shape
    frames = np.stack([L.era5_like(h, w, 40 + s, 1.0 + 0.25 * (s % 3), 0.7 + 0.6 * (s % 2)) for s in range(n)])
    cfg = L.make_config((1, h, w), base_cr=30.0, error=err, residual_type=mode)
    got = {}
    for name, env in (("table", {}), ("walk", {"EBCC_HIP_RATE_WALK": "1"}),
                      ("table, speculation", {"EBCC_HIP_SPECULATION": "1"}),
                      ("walk, speculation", {"EBCC_HIP_RATE_WALK": "1", "EBCC_HIP_SPECULATION": "1"}),
                      ("table, no speculation", {"EBCC_HIP_SPECULATION": "0"})):
        _env(monkeypatch, env)
        with L.Context(n, h, w) as ctx:
            got[name] = ctx.encode_frames(frames, cfg)
    assert all(v == got["walk"] for v in got.values()), [k for k, v in got.items() if v != got["walk"]]
    assert all(len(s) > 0 for s in got["table"])


def test_engine_reuse_rebuilds_the_tables(monkeypatch):
    """a second batch of other frames on a used context gets what a fresh context gives it"""
    _env(monkeypatch, {})
    h, w = 100, 130
    first = np.stack([L.era5_like(h, w, 5 + s) for s in range(3)])
    second = np.stack([L.era5_like(h, w, 90 + s, 1.0, 0.7) for s in range(3)])
    cfg = L.make_config((1, h, w), base_cr=30.0, error=0.05, residual_type=L.MAX_ERROR)
    crs = [7.5, 30.0, 120.0]
    with L.Context(3, h, w) as ctx:
        ctx.j2k_encode(first, crs)
        used_j2k = ctx.j2k_encode(second, crs)[0]
        ctx.encode_frames(first, cfg)
        used = ctx.encode_frames(second, cfg)
        used_short = ctx.encode_frames(second[:2], cfg)                 # (fewer frames than the batch before)
    with L.Context(3, h, w) as ctx:
        fresh_j2k = ctx.j2k_encode(second, crs)[0]
        fresh = ctx.encode_frames(second, cfg)
    assert used_j2k == fresh_j2k
    assert used == fresh and used_short == fresh[:2]
    u16 = [L.scale_u16(f)[0] for f in second]
    assert [L.orc_j2k_encode(u16[f], crs[f]) for f in range(3)] == fresh_j2k
