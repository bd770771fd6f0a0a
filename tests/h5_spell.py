"""Run under an interpreter that has h5py with HDF5_PLUGIN_PATH=<repo>/ebcc_amd: h5_batch.spell_frames on a dataset against the
same loop - step after step in order, as include/ebcc_hip.h states the rule - over h5_batch.read_frames.  Prints 'OK' lines;
tests/test_spell_gpu.py drives it."""
import os
import sys

import h5py
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ebcc_amd import h5_batch  # noqa: E402

out = sys.argv[1]
H, W = 64, 96
NO_STEP = 0xFFFFFFFF
THRESHOLD, MIN_LEN = 280.0, 2
MOVES = [0, 24, 24, 3, 3, 24, 3, 3, 3, 24, 24, 3]                  # columns the wave moves before each step (24: half a period)
row, col = np.mgrid[0:H, 0:W]
shift = np.cumsum(MOVES)
data = np.stack([280 + 12 * np.sin(2 * np.pi * (col - shift[t]) / 48.0 + row / 20.0) + np.random.default_rng(70 + t).normal(0, 0.3, (H, W))
                 for t in range(12)]).astype(np.float32).reshape(2, 6, H, W)
opt = ("relative_error_target", 0.004)
COUNTERS = ("run", "longest", "spells", "spell_steps", "events")
LABELS = ("longest_end", "first", "last", "when_min", "when_max")


def loop(fields, bins, n_bins, when, fresh, below=False, order=None):
    """the spell statistics of fields [n][rows][cols] (float32), step after step"""
    shape = (n_bins,) + fields.shape[1:]
    r = {name: np.zeros(shape, np.uint32) for name in COUNTERS}
    r.update({name: np.full(shape, NO_STEP, np.uint32) for name in LABELS})
    r.update({"min": np.full(shape, np.inf, np.float32), "max": np.full(shape, -np.inf, np.float32), "count": np.zeros(n_bins, np.uint64)})
    for t in (range(len(fields)) if order is None else order):
        k = int(bins[t])
        if k < 0:
            continue
        x, w = fields[t], np.uint32(when[t])
        e = x < np.float32(THRESHOLD) if below else x > np.float32(THRESHOLD)
        run = np.zeros(shape[1:], np.uint32) if fresh[t] else r["run"][k]
        run = np.where(e, run + np.uint32(1), np.uint32(0)).astype(np.uint32)
        r["run"][k] = run
        up = run > r["longest"][k]
        r["longest"][k], r["longest_end"][k] = np.where(up, run, r["longest"][k]), np.where(up, w, r["longest_end"][k])
        r["spells"][k] += run == MIN_LEN
        r["spell_steps"][k] += np.where(run == MIN_LEN, np.uint32(MIN_LEN), np.uint32(0)) + (run > MIN_LEN)
        r["events"][k] += e
        r["first"][k] = np.where(e & (r["first"][k] == NO_STEP), w, r["first"][k])
        r["last"][k] = np.where(e, w, r["last"][k])
        hi, lo = x > r["max"][k], x < r["min"][k]
        r["max"][k], r["when_max"][k] = np.where(hi, x, r["max"][k]), np.where(hi, w, r["when_max"][k])
        r["min"][k], r["when_min"][k] = np.where(lo, x, r["min"][k]), np.where(lo, w, r["when_min"][k])
        r["count"][k] += 1
    r["min"], r["max"] = r["min"] + np.float32(0), r["max"] + np.float32(0)
    return r


def same(got, want, names=COUNTERS + LABELS + ("min", "max", "count")):
    for name in names:
        assert getattr(got, name).tobytes() == want[name].tobytes(), name


with h5py.File(os.path.join(out, "s.h5"), "w") as f, h5_batch.BatchCodec(H, W, max_frames=4) as codec:
    d = h5_batch.create_dataset(f, "t2m", data.shape, 20, opt)
    h5_batch.write_frames(d, data, 20, opt, codec=codec)
with h5py.File(os.path.join(out, "s.h5"), "r") as f, h5_batch.BatchCodec(H, W, max_frames=5) as codec:
    fields = h5_batch.read_frames(f["t2m"], codec=codec)
    flat = fields.reshape(-1, H, W)
    zeros, index, none = np.zeros(12, int), np.arange(12), np.zeros(12, bool)
    want = loop(flat, zeros, 1, index, none)
    # the order of the steps shows: folded backwards the open runs and the labels are other bytes
    back = loop(flat, zeros, 1, index, none, order=range(11, -1, -1))
    assert all(want[name].tobytes() != back[name].tobytes() for name in ("run", "longest_end", "first", "last"))
    assert want["longest"].max() > MIN_LEN and (want["spells"] > 1).any() and (want["spell_steps"] > MIN_LEN * want["spells"]).any()
    got = h5_batch.spell_frames(f["t2m"], THRESHOLD, min_len=MIN_LEN, codec=codec)      # (capacity 5: three batches)
    same(got, want)
    print("OK spell_frames == the loop over read_frames (one bin, whole frames, the default labels)")

    bins = np.broadcast_to(np.array([0, 0, 1, 1, 0, 0]), (2, 6)).copy()
    bins[1, 3] = -1
    when = (np.arange(12) * 37 % 101 + 1000).reshape(2, 6)
    fresh = np.zeros((2, 6), bool)
    fresh[:, 0] = fresh[:, 2] = fresh[1, 4] = True                  # (every visit but the second one of row 0 to bin 0)
    rows, cols = slice(9, 49), slice(50, 80)
    crop = np.ascontiguousarray(fields[..., rows, cols]).reshape(-1, 40, 30)
    want = loop(crop, bins.reshape(-1), 3, when.reshape(-1), fresh.reshape(-1), below=True)
    assert want["longest"].tobytes() != loop(crop, bins.reshape(-1), 3, when.reshape(-1), none, below=True)["longest"].tobytes()
    batches_a_call = h5_batch._SUPER
    try:
        h5_batch._SUPER = 1                                          # (five steps a call: the state, open runs included, is carried over three calls)
        got = h5_batch.spell_frames(f["t2m"], THRESHOLD, below=True, min_len=MIN_LEN, bins=bins, when=when, fresh=fresh, n_bins=3, rows=rows,
                                    cols=cols, codec=codec)
    finally:
        h5_batch._SUPER = batches_a_call
    same(got, want)
    same(h5_batch.spell_frames(f["t2m"], THRESHOLD, below=True, min_len=MIN_LEN, bins=bins, when=when, fresh=fresh, n_bins=3, rows=rows, cols=cols), want)
    assert got.count.tolist() == [8, 3, 0] and (got.first[2] == NO_STEP).all() and got.masked("first")[2].mask.all()
    only = h5_batch.spell_frames(f["t2m"], THRESHOLD, what=("extremes",), codec=codec)
    same(only, loop(flat, zeros, 1, index, none), ("min", "max", "when_min", "when_max", "count"))
    assert only.run is None and only.events is None
    print("OK bins with a skipped step, labels, fresh flags, below and a window: every array equals the loop over read_frames()[..., rows, cols]")

    for bad in [dict(bins=np.zeros(12, int)), dict(bins=np.full((2, 6), -1)), dict(bins=bins, n_bins=1), dict(bins=bins - 2),
                dict(bins=bins.astype(np.float32)), dict(rows=slice(0, 0)), dict(when=np.arange(12)), dict(when=when.astype(np.float32)),
                dict(fresh=np.zeros(12, bool)), dict(what=("spells",))]:
        try:
            h5_batch.spell_frames(f["t2m"], THRESHOLD, codec=codec, **bad)
        except ValueError:
            continue
        raise AssertionError(f"accepted {bad}")
    print("OK bad bins, labels, flags and families are refused")
