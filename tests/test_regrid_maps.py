"""CPU tests of the map builders of ebcc_amd/regrid.py and of the numpy restatement of the regrid rule (tests/_regrid.py): the
weights of means and conservative maps sum to 1, the identity returns its input, a conservative map conserves the integral,
cells across the seam of a periodic axis get wrapping supports, and a destination cell the source does not cover is an error.

ulp: of 1.0, 2^-52.  A block's weights are w / fsum(w): each is within half an ulp of its own value, and their sum of at most
256 terms, taken with math.fsum, is rounded once - 4 ulp holds every case here with room."""
import math

import numpy as np
import pytest

from ebcc_amd import regrid as M
from tests import _regrid as R

ULP = 2.0 ** -52
LAT = np.linspace(90.0, -90.0, 721)
LON = np.arange(1440) * 0.25
LAT1 = np.linspace(90.0, -90.0, 181)
LON1 = np.arange(360) * 1.0


def band(e):
    return np.sin(np.deg2rad(e))


def era5_maps():
    rows = M.conservative_map(M.cell_edges(LAT, -90, 90), M.cell_edges(LAT1, -90, 90), measure=band)
    cols = M.conservative_map(M.cell_edges(LON), M.cell_edges(LON1), period=360.0)
    return rows, cols


def row_sums(m):
    return np.array([math.fsum(m.weights_of(i).tolist()) for i in range(m.n_out)])


def test_rows_of_means_and_conservative_maps_sum_to_one():
    rows, cols = era5_maps()
    maps = [rows, cols, M.block_mean_map(777, 7), M.block_mean_map(130, 4), M.block_mean_map(721, 4, weights=np.cos(np.deg2rad(LAT)) + 1e-3),
            M.conservative_map(np.linspace(0, 777, 778), np.linspace(0, 777, 101)), M.conservative_map(np.arange(65.0), np.linspace(10.0, 50.0, 9))]
    for m in maps:
        assert np.abs(row_sums(m) - 1.0).max() <= 4 * ULP
        assert (m.weight > 0).all()


def test_block_means():
    m = M.block_mean_map(10, 4)
    assert m.first.tolist() == [0, 4, 8] and m.count.tolist() == [4, 4, 2] and not m.wrap      # a ragged end
    assert m.weight.tolist() == [0.25] * 8 + [0.5] * 2
    w = np.array([1.0, 3.0, 0.0, 4.0, 2.0])
    m = M.block_mean_map(5, 2, weights=w)
    assert m.weight.tolist() == [0.25, 0.75, 0.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        M.block_mean_map(4, 2, weights=[1.0, 1.0, 0.0, 0.0])                       # a block without weight
    with pytest.raises(ValueError):
        M.block_mean_map(600, 257)


def test_identity_and_flip_by_the_restatement():
    r = np.random.default_rng(3)
    x = (r.standard_normal((2, 9, 14)) * 1e3).astype(np.float32)
    assert R.apply(x, M.identity_map(9), M.identity_map(14)).tobytes() == x.tobytes()
    assert R.apply(x, M.flip_map(9), M.identity_map(14)).tobytes() == x[:, ::-1].tobytes()
    assert R.apply(x, M.flip_map(9), M.flip_map(14)).tobytes() == x[:, ::-1, ::-1].tobytes()
    # a sample of -0 leaves as +0: t = +0.0 + (-0.0) * 1.0 is +0.0 by the rule
    x[0, 0, 0] = -0.0
    assert R.apply(x, M.identity_map(9), M.identity_map(14)).tobytes() == (x + np.float32(0.0)).tobytes() != x.tobytes()


def test_restatement_against_a_plain_loop():
    """the padded, vectorised form against the two loops of the header, tap by tap, on maps of unequal supports"""
    r = np.random.default_rng(5)
    x = R.items(12, 10, 2)
    rows = M.AxisMap([0, 4, 8], [4, 3, 4], [0.25] * 4 + [0.5, 0.25, 0.25] + [0.25] * 4)
    cols = M.AxisMap([8, 0, 3], [4, 4, 5], [1.0, 0.5, 0.25, 1.0] + [1.0] * 4 + [1.0, 0.5, 0.25, 0.125, -2.0], wrap=True)
    want = np.zeros((2, rows.n_out, cols.n_out), np.float32)
    for k in range(2):
        for R_ in range(rows.n_out):
            for C in range(cols.n_out):
                a = 0.0
                for i, wr in enumerate(rows.weights_of(R_)):
                    t = 0.0
                    for j, wc in enumerate(cols.weights_of(C)):
                        t = t + float(x[k, rows.first[R_] + i, (cols.first[C] + j) % 10]) * float(wc)
                    a = a + float(wr) * t
                want[k, R_, C] = np.float32(a)
    assert R.apply(x, rows, cols).tobytes() == want.tobytes()
    assert R.order_is_visible(x, rows, cols)


def test_conservation_on_the_era5_grids():
    """sum_dst M_dst (W x) == sum_src M_src x on 721 x 1440 -> 181 x 360, both sides by math.fsum on a random float64 field.
    Tolerance 1e-12 relative to sum M |x|: each weight carries a few ulp of 2^-52 and fsum adds nothing."""
    rows, cols = era5_maps()
    assert (rows.n_out, cols.n_out) == (181, 360)
    x = np.random.default_rng(11).standard_normal((721, 1440))
    m_src = np.abs(np.diff(band(M.cell_edges(LAT, -90, 90))))[:, None] * np.abs(np.diff(M.cell_edges(LON)))[None, :]
    m_dst = np.abs(np.diff(band(M.cell_edges(LAT1, -90, 90))))[:, None] * np.abs(np.diff(M.cell_edges(LON1)))[None, :]
    ir, wr = R.padded(rows, 721)
    ic, wc = R.padded(cols, 1440)
    t = (x[:, ic] * wc[None]).sum(axis=2)                               # [721][360]
    y = (t[ir] * wr[:, :, None]).sum(axis=1)                            # [181][360]
    lhs, rhs = math.fsum((m_dst * y).ravel().tolist()), math.fsum((m_src * x).ravel().tolist())
    scale = math.fsum((m_src * np.abs(x)).ravel().tolist())
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)
    # and a constant stays that constant to rounding
    assert np.abs(R.apply(np.full((1, 721, 1440), 273.15, np.float32), rows, cols) - np.float32(273.15)).max() <= 273.15 * 2.0 ** -22


def test_wrapping_supports_across_the_seam():
    rows, cols = era5_maps()
    assert cols.wrap and not rows.wrap
    # destination cell 0 is [-0.5, 0.5]: source cells 1438, 1439 (half of 1438), 0, 1, 2 (half of 2)
    assert int(cols.first[0]) == 1438 and int(cols.count[0]) == 5
    assert np.allclose(cols.weights_of(0), [0.125, 0.25, 0.25, 0.25, 0.125], rtol=0, atol=1e-12)
    assert ((cols.first.astype(np.int64) + cols.count) > 1440).sum() == 1          # the only cell across the seam
    assert int(cols.first[1]) == 2 and int(cols.count[1]) == 5
    # a destination grid shifted by half the period: its cells are taken modulo the period
    shifted = M.conservative_map(M.cell_edges(LON), M.cell_edges(LON1 - 180.0), period=360.0)
    assert shifted.first.tolist() == np.roll(cols.first, 180).tolist() and shifted.wrap
    # linear interpolation across the seam: between the last centre and the first
    lin = M.linear_map(LON, [359.875, 0.0, 0.125], period=360.0)
    assert lin.first.tolist() == [1439, 0, 0] and lin.wrap and lin.weight.tolist() == [0.5, 0.5, 1.0, 0.0, 0.5, 0.5]
    assert not M.linear_map(LON, [10.0, 20.1], period=360.0).wrap


def test_linear_maps_and_edges():
    m = M.linear_map([0.0, 1.0, 3.0], [0.0, 0.25, 2.0, 3.0])
    assert m.first.tolist() == [0, 0, 1, 1] and m.count.tolist() == [2] * 4
    assert m.weight.tolist() == [1.0, 0.0, 0.75, 0.25, 0.5, 0.5, 0.0, 1.0]
    down = M.linear_map([3.0, 1.0, 0.0], [2.0])                                  # decreasing centres
    assert down.first.tolist() == [0] and down.weight.tolist() == [0.5, 0.5]
    with pytest.raises(ValueError):
        M.linear_map([0.0, 1.0], [1.5])
    e = M.cell_edges(LAT, -90, 90)
    assert e[0] == 90.0 and e[-1] == -90.0 and e[1] == 89.875 and len(e) == 722    # pole-centred: clipped at the poles
    assert M.cell_edges(LON)[0] == -0.125 and M.cell_edges(LON)[-1] == 359.875


def test_an_uncovered_destination_cell_raises():
    with pytest.raises(ValueError, match="meets no source cell"):
        M.conservative_map(np.arange(11.0), np.array([8.0, 10.0, 12.0]))           # the last cell lies beyond the source
    with pytest.raises(ValueError, match="meets no source cell"):
        M.conservative_map(np.arange(11.0), np.array([-3.0, -1.0, 4.0]))
    partly = M.conservative_map(np.arange(11.0), np.array([-1.0, 1.0, 12.0]))      # partly covered: normalised by what is covered
    assert partly.first.tolist() == [0, 1] and partly.count.tolist() == [1, 9] and abs(row_sums(partly) - 1).max() <= 4 * ULP
