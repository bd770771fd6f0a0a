"""The child process of tests/test_quantile_threads_gpu.py: `python -m tests._quantile_threads` runs two threads that call
ebcc_hip_quantile_shard (and ebcc_hip_rank_items) on ONE context at once, with specs of different sizes.

The shape is that of tests/_threads.py: the expected planes first, serially, by numpy on the oracle's decode; the threads behind
one barrier, a fixed number of calls each; the comparison after the joins, by bytes.  The larger spec runs once serially before
the threads start, and so does the unit-level call - both are held against numpy there - so the context's workspace already has
its largest size: overlapping calls could then only mix their counters, which the comparison shows as wrong bytes."""
import numpy as np

from tests import _lib as L
from tests import _threads as TH
from tests import test_quantile_gpu as Q

H, W = 64, 96
ROUNDS = 3


def shared_context_two_sizes():
    Q.lib()                                                          # (argument types declared once, before any thread calls)
    streams, fields = Q.series(H, W, 12)
    big_ranks = [[0, 3], [1, Q.NO_RANK], [2, 1]]                     # three bins of whole frames: the larger workspace
    win = (8, 16, 24, 40)
    small_ranks, small_bins = [[1, 4]], [0 if f % 2 else Q.NO_BIN for f in range(12)]
    kept = [f for f in range(12) if small_bins[f] != Q.NO_BIN]
    crop = np.ascontiguousarray(fields[kept][:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    want_big = Q.expected(fields, Q.BINS12, big_ranks)
    want_small = Q.expected(crop, None, small_ranks)
    want_items = Q.expected(fields[:5], Q.KERNEL_BINS, Q.KERNEL_RANKS)
    got = {"big": [], "small": [], "items": []}
    with L.Context(5, H, W) as ctx:                                  # (three batches on two engine sets per pass)
        serial = Q.Ranks(big_ranks, H, W)
        assert Q.quantile(ctx, streams, Q.BINS12, serial) == 0, TH.last_error()
        assert serial.get().tobytes() == want_big[0].tobytes(), "serial product planes differ from numpy on the oracle's decode"
        items = Q.Guarded(np.array(fields[:5]), 1)
        unit = Q.Ranks(Q.KERNEL_RANKS, H, W)                         # (four bins x three slots of whole frames: the largest)
        assert Q.rank_items(ctx, items, Q.KERNEL_BINS, unit) == 0, TH.last_error()
        assert unit.get().tobytes() == want_items[0].tobytes(), "serial product planes of the kernels alone differ from numpy"
        TH.serial_ok()

        def big(barrier):
            for _ in range(ROUNDS):
                spec = Q.Ranks(big_ranks, H, W, base=1)
                rc = Q.quantile(ctx, streams, Q.BINS12, spec)
                got["big"].append((rc, spec.get().tobytes(), spec.count.tolist(), spec.out.sentinels_intact()))

        def small(barrier):
            for _ in range(ROUNDS):
                spec = Q.Ranks(small_ranks, win[2], win[3])
                rc = Q.quantile(ctx, streams, small_bins, spec, win[0], win[1])
                got["small"].append((rc, spec.get().tobytes(), spec.count.tolist(), spec.out.sentinels_intact()))
                unit = Q.Ranks(Q.KERNEL_RANKS, H, W)
                rc = Q.rank_items(ctx, items, Q.KERNEL_BINS, unit)
                got["items"].append((rc, unit.get().tobytes(), unit.count.tolist(), unit.out.sentinels_intact()))

        TH.run_threads([big, small])
        assert items.untouched()
    for name, want in (("big", want_big), ("small", want_small), ("items", want_items)):
        assert len(got[name]) == ROUNDS
        for r, (rc, planes, count, intact) in enumerate(got[name]):
            assert rc == 0 and intact, (name, r, rc)
            assert planes == want[0].tobytes(), (name, r, "planes selected beside another quantile call on the context differ")
            assert count == want[1].tolist(), (name, r)


if __name__ == "__main__":
    L.oracle().orc_set_j2k_backend(0)
    shared_context_two_sizes()
    TH.say("compared")
