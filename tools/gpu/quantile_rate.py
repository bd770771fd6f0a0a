"""GPU box: what the quantile decode costs on the bench workload ("Quantile decode").
256 frames of 721x1440 from the bench's field generator, coded with base_cr 30 and MAX_ERROR 0.5 and resident as streams, a
context of 256 frames.
  a  ebcc_hip_reduce_shard with one bin and d_min only, the parent's library (--parent-lib) and this build - the yardstick: one
     decode plus one streaming pass over the decoded batch; beside it the same for the regional box
  b  ebcc_hip_quantile_shard, one bin, the ranks of the 5 %, 50 % and 95 % points, whole frames
  c  the same for the 200 x 300 box at (260, 570)
  d  12 bins (frame % 12) x 3 ranks, whole frames (a workspace of 2.7 GB)
  e  the kernels alone (ebcc_hip_rank_items on the decoded frames, timed with events: ebcc_hip_timing_read "rank_count" /
     "rank_advance"), per pass, in GB/s of the frames read
ms are the median of --reps calls after one warm-up.  Every run asserts that rows b to d are, byte for byte,
ebcc_hip_rank_items of what ebcc_hip_decode_shard gave.  A quantile call is eight passes, so each row is set against eight
times the parent's row a of the same round.

    python tools/gpu/quantile_rate.py [--parent-lib PATH] [--rounds 2] [--reps 5]

Every measurement is a child process under its own time limit, the two libraries alternate, and nothing more is started after a
child fails."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N = 256
CHILD_LIMIT = 300
BOX = (260, 570, 200, 300)                             # row0, col0, rows, cols
PASSES = 8


def med(v):
    return sorted(v)[len(v) // 2]


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from tests import _lib as L
    if args.lib:
        L.PRODUCT_SO = args.lib
    lib = L.product()
    import bench
    from ebcc_amd import h5_batch as B
    H, W = bench.H, bench.W
    dev = torch.device("cuda", 0)
    frames = bench.synth_frames(torch, N, dev, seed=0)
    torch.cuda.synchronize()
    ctx = L.Context(N, H, W)
    lib.ebcc_hip_prepare.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert lib.ebcc_hip_prepare(ctx.ptr, N) == 0
    cfg = L.make_config((1, H, W), base_cr=bench.BASE_CR, error=bench.MAX_ERR, residual_type=L.MAX_ERROR)
    outs, sizes = (ctypes.c_void_p * N)(), (ctypes.c_size_t * N)()
    assert lib.ebcc_hip_encode_shard(ctx.ptr, frames.data_ptr(), N, ctypes.byref(cfg), outs, sizes) == 0, lib.ebcc_hip_last_error()
    lib.ebcc_hip_time_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(B.TimeStats)]
    lib.ebcc_hip_reduce_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.POINTER(B.TimeStats)]

    def timed(call):
        assert call() == 0, lib.ebcc_hip_last_error()                     # (warm-up)
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rc = call()
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
            assert rc == 0, lib.ebcc_hip_last_error()
        return ms

    res = {}
    count = np.zeros(12, np.uint64)
    for key, (row0, col0, rows, cols) in (("whole", (0, 0, H, W)), ("box", BOX)):
        mn = torch.empty((rows, cols), dtype=torch.float32, device=dev)
        st = B.TimeStats(1, rows, cols, None, None, mn.data_ptr(), None, None, 0.0, count.ctypes.data)
        assert lib.ebcc_hip_time_stats_init(ctx.ptr, ctypes.byref(st)) == 0
        res[f"reduce_{key}_ms"] = timed(lambda: lib.ebcc_hip_reduce_shard(ctx.ptr, outs, sizes, N, None, row0, col0, ctypes.byref(st)))
    if not args.parent:
        lib.ebcc_hip_rank_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(B.TimeRanks)]
        lib.ebcc_hip_quantile_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                ctypes.POINTER(B.TimeRanks)]
        lib.ebcc_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.ebcc_hip_timing_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        dec = torch.empty_like(frames)
        assert lib.ebcc_hip_decode_shard(ctx.ptr, outs, sizes, N, dec.data_ptr()) == 0, lib.ebcc_hip_last_error()

        def events(call):
            lib.ebcc_hip_timing_enable(ctx.ptr, 1)
            for _ in range(args.reps):
                assert call() == 0
            got = {}
            for name in (b"rank_count", b"rank_advance"):
                total, launches = ctypes.c_double(), ctypes.c_long()
                lib.ebcc_hip_timing_read(ctx.ptr, name, ctypes.byref(total), ctypes.byref(launches))
                got[name.decode()] = total.value / (args.reps * PASSES)          # per pass
            lib.ebcc_hip_timing_enable(ctx.ptr, 0)
            return got

        one = [int(round(q * (N - 1))) for q in (0.05, 0.5, 0.95)]
        month = (np.arange(N) % 12).astype(np.uint32)
        per_month = int(np.bincount(month).min())
        twelve = [[int(round(q * (per_month - 1))) for q in (0.05, 0.5, 0.95)]] * 12
        for key, (row0, col0, rows, cols), ranks, bins in (("one", (0, 0, H, W), [one], None), ("box", BOX, [one], None), ("months", (0, 0, H, W), twelve, month)):
            table = np.ascontiguousarray(np.asarray(ranks, np.uint64))
            shape = table.shape + (rows, cols)
            got = torch.empty(shape, dtype=torch.float32, device=dev)
            ref = torch.empty(shape, dtype=torch.float32, device=dev)
            bp = None if bins is None else bins.ctypes.data
            spec = B.TimeRanks(shape[0], rows, cols, shape[1], table.ctypes.data, got.data_ptr(), count.ctypes.data)
            res[f"quantile_{key}_ms"] = timed(lambda: lib.ebcc_hip_quantile_shard(ctx.ptr, outs, sizes, N, bp, row0, col0, ctypes.byref(spec)))
            crop = dec if key != "box" else dec[:, row0:row0 + rows, col0:col0 + cols].contiguous()
            rspec = B.TimeRanks(shape[0], rows, cols, shape[1], table.ctypes.data, ref.data_ptr(), count.ctypes.data)
            items = lambda: lib.ebcc_hip_rank_items(ctx.ptr, crop.data_ptr(), N, bp, ctypes.byref(rspec))  # noqa: E731
            res[f"items_{key}_call_ms"] = timed(items)
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{key}: the quantile decode and the kernels on the decoded frames disagree"
            ev = events(items)
            res[f"items_{key}_count_ms"], res[f"items_{key}_advance_ms"] = ev["rank_count"], ev["rank_advance"]
            res[f"items_{key}_gb_s"] = N * rows * cols * 4 / (ev["rank_count"] * 1e-3) / 1e9
            del got, ref
    for i in range(N):
        lib.free_buffer(outs[i])
    ctx.close()
    print("QUANTILE_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("QUANTILE_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    return json.loads(line[0].split(" ", 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: its reduce decode is the yardstick")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--parent", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    common = ["--reps", str(args.reps)]
    for rnd in range(args.rounds):
        a = None
        if args.parent_lib:
            a = run_child(common + ["--parent", "--lib", os.path.abspath(args.parent_lib)])
            print(f"round {rnd} [parent]     a reduce_shard, one bin, d_min: whole frames {med(a['reduce_whole_ms']):8.2f} ms {a['reduce_whole_ms']}; "
                  f"the box {med(a['reduce_box_ms']):.2f} ms {a['reduce_box_ms']}", flush=True)
        b = run_child(common)
        print(f"round {rnd} [this build] a reduce_shard, one bin, d_min: whole frames {med(b['reduce_whole_ms']):8.2f} ms {b['reduce_whole_ms']}; "
              f"the box {med(b['reduce_box_ms']):.2f} ms {b['reduce_box_ms']}", flush=True)
        for row, key, what in (("b", "one", "one bin x 3 ranks, whole frames"), ("c", "box", "one bin x 3 ranks, the box"), ("d", "months", "12 bins x 3 ranks, whole frames")):
            print(f"round {rnd} [this build] {row} quantile_shard, {what}: {med(b[f'quantile_{key}_ms']):8.2f} ms {b[f'quantile_{key}_ms']}", flush=True)
            print(f"round {rnd} [this build] e rank_items on the decoded frames, {what}: call {med(b[f'items_{key}_call_ms']):.2f} ms; per pass: rank_count "
                  f"{b[f'items_{key}_count_ms']:.3f} ms = {b[f'items_{key}_gb_s']:.0f} GB/s of the frames read, rank_advance {b[f'items_{key}_advance_ms']:.3f} ms", flush=True)
        y = a if a is not None else b
        for row, key, base in (("b", "one", "reduce_whole_ms"), ("c", "box", "reduce_box_ms"), ("d", "months", "reduce_whole_ms")):
            eight = PASSES * med(y[base])
            print(f"round {rnd} row {row}: {med(b[f'quantile_{key}_ms']):.2f} ms against 8 x {'the parent' if a is not None else 'this build'}'s row a = {eight:.2f} ms: "
                  f"x {med(b[f'quantile_{key}_ms']) / eight:.2f}", flush=True)


if __name__ == "__main__":
    main()
