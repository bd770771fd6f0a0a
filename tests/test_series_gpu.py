"""GPU: the area series of include/ebcc_hip.h - ebcc_hip_area_fold (k_area_rows and k_area_fold alone) on numpy's own arrays and
ebcc_hip_series_shard on streams, against the numpy restatement of the header's fold (tests/_series.py) applied to the arrays or
to the oracle's decode of the same streams.  Everything is compared by tobytes(): there is no tolerance in this file.  The
inputs make the order of the additions visible - blocks of rows and columns differ in scale by factors of 1e6, so a float64 sum
rounds - and every test that relies on that first asserts that its own expected sums differ from a plain left-to-right loop.

The launches of area_fold are cut by one count limit, 2^18 records a launch: the items of a call into runs, the regions of a
list into groups.  test_launch_limits drives both past it.

Not tested here: the refusal of a context for chunks of several frames - the C interface has no call that makes one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _hard_bound as HB
from tests import _lib as L
from tests import _series as S
from tests import test_reduce_gpu as RG
from tests import test_window_gpu as T

pytestmark = pytest.mark.gpu

Guarded = RG.Guarded
SCALES = RG.SCALES
THRESHOLD = 5.0
JUNK = 0xA5                                           # what `out` holds before a call
MARGIN = 4                                            # records of junk before and behind `out`


def lib():
    """the product with the area entry points declared (an AttributeError where they are missing: a failure, not a skip)"""
    p = RG.lib()                                      # (ebcc_hip_window_plan is declared there)
    p.ebcc_hip_area_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(S.AreaSpec),
                                     ctypes.c_void_p]
    p.ebcc_hip_series_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.POINTER(S.AreaSpec), ctypes.c_void_p]
    for name in ("ebcc_hip_area_fold", "ebcc_hip_series_shard"):
        getattr(p, name).restype = ctypes.c_int
    return p


@pytest.fixture(autouse=True)
def _entry_points():
    lib()


last_error = RG.last_error


class Out:
    """the host records [n][R] between margins of junk"""

    def __init__(self, n, n_regions):
        self.buf = np.full((n * n_regions + 2 * MARGIN) * S.AREA_STAT.itemsize, JUNK, np.uint8)
        self.body = self.buf[MARGIN * 32:(MARGIN + n * n_regions) * 32]
        self.shape = (n, n_regions)

    @property
    def ptr(self):
        return self.body.ctypes.data

    def get(self):
        return self.body.view(S.AREA_STAT).reshape(self.shape).copy()

    def margins_intact(self):
        return bool((self.buf[:MARGIN * 32] == JUNK).all() and (self.buf[self.buf.size - MARGIN * 32:] == JUNK).all())

    def untouched(self):
        return bool((self.buf == JUNK).all())


def make_spec(regions, w_row, w_pix, threshold):
    """-> (AreaSpec, what it points to); w_pix: a Guarded or None"""
    arr = S.region_array(regions)
    wr = None if w_row is None else np.ascontiguousarray(w_row, np.float64)
    spec = S.AreaSpec(len(regions), ctypes.addressof(arr), None if wr is None else wr.ctypes.data, None if w_pix is None else w_pix.ptr,
                      0 if threshold is None else 1, 0.0 if threshold is None else threshold)
    return spec, (arr, wr)


def fold(ctx, items, regions, w_row=None, w_pix=None, threshold=None, out=None):
    """ebcc_hip_area_fold of the Guarded items [n][h][w] -> (status, Out)"""
    n, h, w = items.shape
    out = out or Out(n, len(regions))
    spec, keep = make_spec(regions, w_row, w_pix, threshold)
    rc = lib().ebcc_hip_area_fold(ctx.ptr, items.ptr, n, h, w, ctypes.byref(spec), out.ptr)
    return rc, out


def same(got, want, what):
    for name in S.FIELDS:
        assert got[name].tobytes() == want[name].tobytes(), (what, name)


# ---- 1. the kernels alone against numpy ----------------------------------------------------------------------------------
def kernel_items(h, w, n=3):
    """n items of N(5, 3) samples; blocks of two rows and of two columns scaled by 1e-6, 1, 1e6 in turn; -0 planted"""
    r = np.random.default_rng(h * 1000 + w)
    x = (r.standard_normal((n, h, w)) * 3 + 5).astype(np.float32)
    rows, cols = np.arange(h)[:, None], np.arange(w)[None, :]
    x = x * np.asarray(SCALES, np.float32)[(rows // 2 + cols // 2 + 1) % 3][None]
    x[0, 0, 0] = x[1, h - 1, w - 1] = -0.0
    return np.ascontiguousarray(x, np.float32)


def weights(h, w, mode):
    """(w_row, w_pix) for none / row / pix / both: cos(latitude) per row, a land fraction per pixel with a third of it masked"""
    r = np.random.default_rng(h + w)
    w_row = np.cos(np.deg2rad(np.linspace(-89.5, 89.5, h)))
    w_pix = r.random((h, w)).astype(np.float32)
    w_pix[r.random((h, w)) < 0.33] = 0.0
    return (w_row if mode in ("row", "both") else None), (w_pix if mode in ("pix", "both") else None)


# widths 1, 3, 4, 5, 255, 256, 257, 260, 513, 777 at the left edge, the right edge and odd columns; heights 1 .. 5
REGIONS_WIDE = [(0, 0, 5, 777), (0, 0, 1, 1), (4, 776, 1, 1), (1, 3, 2, 3), (0, 773, 5, 4), (2, 1, 1, 5), (0, 0, 3, 255), (1, 522, 4, 255),
                (0, 7, 5, 256), (3, 521, 2, 256), (0, 2, 1, 257), (1, 520, 1, 257), (0, 517, 5, 260), (2, 0, 2, 513), (0, 264, 5, 513),
                (4, 0, 1, 777), (0, 7, 5, 256), (1, 100, 3, 300)]                 # (0, 7, 5, 256) twice; most of them overlap
# heights 1, 63, 64, 65, 129, 130 at the top and the bottom edge; widths 1 .. 9
REGIONS_TALL = [(0, 0, 130, 9), (0, 0, 1, 9), (129, 0, 1, 9), (0, 0, 63, 1), (67, 8, 63, 1), (0, 2, 64, 4), (66, 5, 64, 4), (1, 1, 65, 7),
                (65, 0, 65, 3), (0, 4, 129, 5), (1, 0, 129, 8), (66, 5, 64, 4), (30, 3, 70, 3)]      # (66, 5, 64, 4) twice
GEOMETRIES = {(5, 777): REGIONS_WIDE, (130, 9): REGIONS_TALL}


@pytest.mark.parametrize("mode", ["none", "row", "pix", "both"])
@pytest.mark.parametrize("h,w", list(GEOMETRIES))
def test_kernels_against_numpy(h, w, mode):
    regions = GEOMETRIES[(h, w)]
    x = kernel_items(h, w)
    w_row, w_pix = weights(h, w, mode)
    whole = (0, 0, h, w)
    assert S.region_stats(x, whole, w_row, w_pix)["sum"].tobytes() != S.left_to_right(x, whole, w_row, w_pix).tobytes()
    visible = sum(S.region_stats(x, r, w_row, w_pix)["sum"].tobytes() != S.left_to_right(x, r, w_row, w_pix).tobytes() for r in regions)
    assert visible >= len(regions) // 2                              # (a region of one column of one scale adds exactly)
    with L.Context(4, 64, 96) as ctx:                                # (any context of the device)
        items = Guarded(x, 1)
        pix = None if w_pix is None else Guarded(w_pix, 3)
        for threshold in (THRESHOLD, None):
            want = S.expected(x, regions, w_row, w_pix, threshold)
            rc, out = fold(ctx, items, regions, w_row, pix, threshold)
            assert rc == 0, last_error()
            got = out.get()
            same(got, want, (h, w, mode, threshold))
            assert out.margins_intact() and items.untouched() and (pix is None or pix.untouched())
            if threshold is None:
                assert not got["over"].any()
            else:
                assert 0 < got["over"][:, 0].min() and (got["over"][:, 0] < S.total_weight([whole], h, w, w_row, w_pix)[0]).all()
        # a region listed twice gives the same bytes twice
        twice = [i for i, r in enumerate(regions) if regions.count(r) == 2]
        assert len(twice) == 2 and got[:, twice[0]].tobytes() == got[:, twice[1]].tobytes()
        # a region alone gives the bytes it gives inside the list; so does the list backwards
        for i, r in enumerate(regions):
            rc, out = fold(ctx, items, [r], w_row, pix, None)
            assert rc == 0 and out.get()[:, 0].tobytes() == got[:, i].tobytes(), r
        rc, out = fold(ctx, items, regions[::-1], w_row, pix, None)
        assert rc == 0 and out.get()[:, ::-1].tobytes() == got.tobytes()
        # a second run: the same bytes
        rc, out = fold(ctx, items, regions, w_row, pix, None)
        assert rc == 0 and out.get().tobytes() == got.tobytes()


def test_results_do_not_depend_on_alignment():
    h, w = 5, 777
    x = kernel_items(h, w)
    w_row, w_pix = weights(h, w, "both")
    seen = set()
    with L.Context(4, 64, 96) as ctx:
        for item_base in range(4):
            for pix_base in range(4):
                rc, out = fold(ctx, Guarded(x, item_base), REGIONS_WIDE, w_row, Guarded(w_pix, pix_base), THRESHOLD)
                assert rc == 0, last_error()
                seen.add(out.get().tobytes())
    assert len(seen) == 1 and seen.pop() == S.expected(x, REGIONS_WIDE, w_row, w_pix, THRESHOLD).tobytes()


def test_masks_and_negative_zero():
    h, w = 9, 21
    x = kernel_items(h, w, 2)
    x[0, 2, 3], x[1, 2, 3] = 9e30, -9e30                             # extremes that the mask hides
    x[:, 6:8, 10:17] = -0.0                                          # a block of -0
    x[0, 6, 12] = 0.0
    mask = np.ones((h, w), np.float32)
    mask[2, 3] = 0.0
    mask[4:6, :] = 0.0                                               # two dead rows
    mask[0, 0] = -0.0                                                # (-0 is 0)
    regions = [(0, 0, h, w), (1, 1, 3, 5), (4, 0, 2, w), (4, 5, 1, 1), (6, 10, 2, 7), (6, 10, 1, 2)]
    want = S.expected(x, regions, None, mask, THRESHOLD)
    with L.Context(4, 64, 96) as ctx:
        rc, out = fold(ctx, Guarded(x, 2), regions, None, Guarded(mask, 1), THRESHOLD)
        assert rc == 0, last_error()
        got = out.get()
    same(got, want, "masks")
    assert np.abs(got["max"][:, :2]).max() < 1e8 and np.abs(got["min"][:, :2]).max() < 1e8      # the masked extremes are not seen
    zero = np.float64(0.0).tobytes()
    for k in range(2):                                               # all-zero regions: +0.0 sums, min = +inf, max = -inf
        for g in (2, 3):
            assert got["sum"][k, g].tobytes() == zero and got["sum_sq"][k, g].tobytes() == zero and got["over"][k, g].tobytes() == zero
            assert got["min"][k, g] == np.inf and got["max"][k, g] == -np.inf
    # -0 counts as +0 and +0 is written: a region of -0 samples alone
    fzero = np.float32(0.0).tobytes()
    for g in (4, 5):
        assert got["min"][1, g].tobytes() == fzero and got["max"][1, g].tobytes() == fzero and got["sum"][1, g].tobytes() == zero


def test_launch_limits():
    """more row records than a launch makes (2^18): the items of a call in runs, the regions of a list in groups"""
    h, w = 2, 5
    w_row = np.array([0.75, 1.0 / 3.0])
    r = np.random.default_rng(7)
    distinct = [(0, 0, 2, 5), (0, 1, 2, 3), (0, 0, 2, 4), (0, 2, 2, 3), (0, 0, 2, 1)]
    with L.Context(4, 64, 96) as ctx:
        # 4097 items x 40 regions of two rows: 327760 row records, two runs of items
        n = 4097
        x = (r.standard_normal((n, h, w)) * 3 + 5).astype(np.float32) * np.asarray(SCALES, np.float32)[np.arange(w) % 3][None, None, :]
        regions = [distinct[i % 5] for i in range(40)]
        assert n * sum(g[2] for g in regions) > 2 ** 18
        base = S.expected(x, distinct, w_row, None, THRESHOLD)
        assert base["sum"][:, 0].tobytes() != S.left_to_right(x, distinct[0], w_row).tobytes()
        items = Guarded(x, 1)
        rc, out = fold(ctx, items, regions, w_row, None, THRESHOLD)
        assert rc == 0, last_error()
        same(out.get(), base[:, np.arange(40) % 5], "runs of items")
        assert out.margins_intact() and items.untouched()
        # 2 items x 131080 regions of two rows: 262160 rows in the list, two groups of regions, each in two runs
        m = 131080
        regions = [distinct[i % 5] for i in range(m)]
        assert sum(g[2] for g in regions) > 2 ** 18
        items = Guarded(x[:2], 0)
        rc, out = fold(ctx, items, regions, w_row, None, THRESHOLD)
        assert rc == 0, last_error()
        same(out.get(), base[:2][:, np.arange(m) % 5], "groups of regions")
        assert out.margins_intact() and items.untouched()


def test_bad_weights_and_bad_arguments_write_nothing():
    h, w = 9, 21
    x = kernel_items(h, w, 2)
    regions = [(1, 1, 3, 5), (2, 4, 6, 10)]                          # bounding box [1, 8) x [1, 14)
    with L.Context(4, 64, 96) as ctx:
        items = Guarded(x, 0)
        for bad in (np.nan, -1.0, np.inf, -np.inf, -1e-30):
            for at in ((1, 1), (7, 13), (4, 6)):
                pix = np.ones((h, w), np.float32)
                pix[at] = bad
                rc, out = fold(ctx, items, regions, None, Guarded(pix, 1))
                assert rc == 1 and last_error() and out.untouched(), (bad, at)
        # a weight no region holds is not looked at
        pix = np.ones((h, w), np.float32)
        pix[0, 0] = pix[8, 20] = pix[1, 14] = pix[8, 1] = np.nan
        rc, out = fold(ctx, items, regions, None, Guarded(pix, 1))
        assert rc == 0, last_error()
        same(out.get(), S.expected(x, regions, None, np.ones((h, w), np.float32)), "weights outside the box")
        # what the check refuses, and bad pointers
        for kw in (dict(regions=[(0, 0, h + 1, w)]), dict(regions=regions, w_row=np.full(h, -1.0))):
            rc, out = fold(ctx, items, **kw)
            assert rc == 1 and last_error() and out.untouched()
        spec, keep = make_spec(regions, None, None, None)
        out = Out(2, 2)
        assert lib().ebcc_hip_area_fold(ctx.ptr, items.ptr + 2, 2, h, w, ctypes.byref(spec), out.ptr) == 1     # items not 4-byte aligned
        assert lib().ebcc_hip_area_fold(ctx.ptr, None, 2, h, w, ctypes.byref(spec), out.ptr) == 1
        assert lib().ebcc_hip_area_fold(ctx.ptr, items.ptr, 0, h, w, ctypes.byref(spec), out.ptr) == 1
        assert lib().ebcc_hip_area_fold(ctx.ptr, items.ptr, 2, h, w, ctypes.byref(spec), None) == 1
        assert out.untouched() and items.untouched()


# ---- 2. streams against the oracle, across batches -------------------------------------------------------------------------
H, W = RG.H, RG.W
CORNER, OPPOSITE = (0, 0, 20, 30), (H - 9, W - 11, 9, 11)
REGIONS = [(0, 0, H, W), CORNER, OPPOSITE, (9, 50, 40, 30), (H - 1, 0, 1, W), CORNER]


def series(ctx, streams, regions, w_row=None, w_pix=None, threshold=None, out=None):
    """ebcc_hip_series_shard -> (status, Out)"""
    keep, ptrs, sizes = RG._args(streams)
    out = out or Out(len(streams), len(regions))
    spec, keep2 = make_spec(regions, w_row, w_pix, threshold)
    return lib().ebcc_hip_series_shard(ctx.ptr, ptrs, sizes, len(streams), ctypes.byref(spec), out.ptr), out


def test_streams_against_the_oracle_across_batches(monkeypatch):
    HB.use_env(monkeypatch, {})
    streams, fields = RG.series(H, W, 12)
    w_row, w_pix = weights(H, W, "both")
    assert S.region_stats(fields, REGIONS[0], w_row, w_pix)["sum"].tobytes() != S.left_to_right(fields, REGIONS[0], w_row, w_pix).tobytes()
    threshold = float(np.median(fields[1]))
    want = S.expected(fields, REGIONS, w_row, w_pix, threshold)
    assert 0 < want["over"][1, 0] < S.total_weight(REGIONS[:1], H, W, w_row, w_pix)[0]
    seen = []
    for cap in (5, 16, 5):                                          # three batches on two engine sets; one batch; the first again
        with L.Context(cap, H, W) as ctx:
            pix = Guarded(w_pix, 1)
            rc, out = series(ctx, streams, REGIONS, w_row, pix, threshold)
            assert rc == 0, last_error()
            same(out.get(), want, f"capacity {cap}")
            assert out.margins_intact() and pix.untouched()
            seen.append(out.get().tobytes())
    assert seen[0] == seen[1] == seen[2]


def test_a_window_gives_the_bytes_of_the_frame(monkeypatch):
    """a corner region alone is decoded as a window; listed with the opposite corner the bounding box is the frame (every
    subband of these small frames is one code-block: test_wide_frames_and_the_fold_of_the_decode has a window that needs fewer
    code-blocks than the frame has)"""
    HB.use_env(monkeypatch, {})
    streams, fields = RG.series(H, W, 12)
    w_row, _ = weights(H, W, "row")
    want = S.expected(fields, [CORNER, OPPOSITE], w_row)
    assert want["sum"][:, 0].tobytes() != S.left_to_right(fields, CORNER, w_row).tobytes()
    with L.Context(5, H, W) as ctx:
        rc, alone = series(ctx, streams, [CORNER], w_row)
        assert rc == 0, last_error()
        rc, both = series(ctx, streams, [CORNER, OPPOSITE], w_row)
        assert rc == 0, last_error()
        rc, other = series(ctx, streams, [OPPOSITE], w_row)
        assert rc == 0, last_error()
    same(both.get(), want, "two corners")
    assert alone.get()[:, 0].tobytes() == both.get()[:, 0].tobytes() and other.get()[:, 0].tobytes() == both.get()[:, 1].tobytes()
    assert alone.margins_intact() and both.margins_intact()


def test_wide_frames_and_the_fold_of_the_decode(monkeypatch):
    """frames wider than 256 columns - a lane takes more than one quad of decoded data -, and the series equals
    ebcc_hip_area_fold of what ebcc_hip_decode_shard returns"""
    HB.use_env(monkeypatch, {})
    h, w = 48, 300
    streams, fields = RG.series(h, w, 5)
    w_row, w_pix = weights(h, w, "both")
    narrow = (5, 250, 10, 41)
    regions = [(0, 0, h, w), (3, 7, 40, 290), (0, 1, 1, 299), (5, 30, 10, 261), narrow]
    n = lib().ebcc_hip_window_plan(h, w, *narrow, None, None, 0)
    blocks = np.zeros((n, 6), np.int32)
    assert n > 0 and lib().ebcc_hip_window_plan(h, w, *narrow, None, blocks.ctypes.data, n) == n
    assert 0 < blocks[:, 5].sum() < n                               # a real window: fewer code-blocks than the frame has
    want = S.expected(fields, regions, w_row, w_pix, THRESHOLD)
    assert want["sum"][:, 0].tobytes() != S.left_to_right(fields, regions[0], w_row, w_pix).tobytes()
    with L.Context(2, h, w) as ctx:                                 # (three batches)
        pix = Guarded(w_pix, 2)
        rc, out = series(ctx, streams, regions, w_row, pix, THRESHOLD)
        assert rc == 0, last_error()
        same(out.get(), want, "wide frames")
        rc, window = series(ctx, streams, regions[1:], w_row, pix, THRESHOLD)        # (the bounding box is a window)
        assert rc == 0, last_error()
        assert window.get().tobytes() == out.get()[:, 1:].tobytes()
        rc, alone = series(ctx, streams, [narrow], w_row, pix, THRESHOLD)            # (from fewer code-blocks)
        assert rc == 0, last_error()
        assert alone.get()[:, 0].tobytes() == out.get()[:, 4].tobytes()
        decoded = ctx.decode_frames(streams, shard=True)
        assert np.array_equal(decoded, fields)
        rc, folded = fold(ctx, Guarded(decoded, 3), regions, w_row, pix, THRESHOLD)
        assert rc == 0, last_error()
        assert folded.get().tobytes() == out.get().tobytes()


def test_refusals_and_a_stream_damaged_inside_a_batch(monkeypatch):
    """What is refused before anything is written, and the damaged stream of tests/test_codec_gpu.py::
    test_malformed_streams_are_rejected (its frame header parses, the decode of its batch refuses it) in the first batch and in
    the last: the call returns 1, nothing outside `out` is written, and the next call on the context is correct."""
    HB.use_env(monkeypatch, {})
    streams, fields = RG.series(H, W, 12)
    want = S.expected(fields, REGIONS, None, None, None)

    def make():
        with L.Context(4, H, W) as ctx:
            return ctx.encode_frames(L.era5_like(H, W, 64)[None], L.make_config((1, H, W), base_cr=10, residual_type=L.NONE))[0][:40]
    damaged = HB.once("reduce damaged stream", make)
    with L.Context(5, 90, 131) as other:                            # a context of another geometry: no region list fits both
        rc, out = series(other, streams, [(0, 0, 90, 131)])
        assert rc == 1 and last_error() and out.margins_intact()
    with L.Context(5, H, W) as ctx:
        cut = list(streams)
        cut[10] = cut[10][:40]                                      # a truncated header, in the last batch
        rc, out = series(ctx, cut, REGIONS)
        assert rc == 1 and last_error() and out.untouched()
        rc, out = series(ctx, [None] + list(streams[1:]), REGIONS)  # a frame without a stream
        assert rc == 1 and last_error() and out.untouched()
        rc, out = series(ctx, streams, [(1, 0, H, W)])              # a region that leaves the frame
        assert rc == 1 and last_error() and out.untouched()
        pix = np.ones((H, W), np.float32)
        pix[H - 1, W - 1] = np.nan
        rc, out = series(ctx, streams, REGIONS, None, Guarded(pix, 0))
        assert rc == 1 and "d_w_pix" in last_error() and out.untouched()
        for at in (1, 11):                                          # in the first batch of three; in the last
            bad = list(streams)
            bad[at] = damaged
            rc, out = series(ctx, bad, REGIONS)
            assert rc == 1 and last_error() and out.margins_intact()
            rc, out = series(ctx, streams, REGIONS)
            assert rc == 0, last_error()
            same(out.get(), want, f"after the damaged stream at {at}")


# ---- 3. h5py -------------------------------------------------------------------------------------------------------------
def test_series_frames_of_a_dataset(tmp_path):
    """h5_batch.BatchCodec.series and h5_batch.series_frames under an interpreter with h5py, as tests/test_reduce_gpu.py drives
    reduce_frames"""
    if not os.path.exists(T.CONDA_PY):
        pytest.skip("no interpreter with h5py in this image")
    if subprocess.call([T.CONDA_PY, "-c", "import h5py"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("h5py not importable")
    env = dict(os.environ, HDF5_PLUGIN_PATH=os.path.join(L.ROOT, "ebcc_amd"), HDF5_USE_FILE_LOCKING="FALSE")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([T.CONDA_PY, os.path.join(L.ROOT, "tests", "h5_series.py"), str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("OK") == 4, r.stdout
