"""GPU box: what the pair decode costs on the bench workload ("Pair decode").
256 steps x 2 variables of 721x1440 from the bench's field generator (seeds 0 and 1), coded with base_cr 30 and MAX_ERROR 0.5
and resident as streams, a context of 256 frames.
  y  two ebcc_hip_reduce_shard calls, one per variable, one bin, d_sum and d_sum_sq - the host-free way to the four plain moments
     before this call existed; the parent's library (--parent-lib) and this build.  The yardstick: the same 512 frames decoded,
     every decoded sample read once.
  1  ebcc_hip_pair_shard, the five co-moments (no magnitude)
  2  ebcc_hip_pair_shard, the magnitude alone (sum, maximum, count above 15)
  3  ebcc_hip_pair_shard, all eight arrays
  k  the kernels alone, timed with events (ebcc_hip_timing_read): "time_fold" summed over the two calls of row y, "pair_fold"
     for rows 1 to 3, per call
ms are the median of --reps calls after one warm-up.  Every run asserts that sum_x / sum_xx / sum_y / sum_yy of row 1 are, byte
for byte, the sums of row y.

    python tools/gpu/pair_rate.py [--parent-lib PATH] [--rounds 2] [--reps 5]

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
CHILD_LIMIT = 400
ROWS = (("1", "moments", "the five co-moments"), ("2", "magnitude", "the magnitude alone"), ("3", "all", "all eight arrays"))


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
    ctx = L.Context(N, H, W)
    lib.ebcc_hip_prepare.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert lib.ebcc_hip_prepare(ctx.ptr, N) == 0
    cfg = L.make_config((1, H, W), base_cr=bench.BASE_CR, error=bench.MAX_ERR, residual_type=L.MAX_ERROR)
    var = []
    for seed in (0, 1):
        frames = bench.synth_frames(torch, N, dev, seed=seed)
        torch.cuda.synchronize()
        outs, sizes = (ctypes.c_void_p * N)(), (ctypes.c_size_t * N)()
        assert lib.ebcc_hip_encode_shard(ctx.ptr, frames.data_ptr(), N, ctypes.byref(cfg), outs, sizes) == 0, lib.ebcc_hip_last_error()
        var.append((outs, sizes))
        del frames
    lib.ebcc_hip_time_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(B.TimeStats)]
    lib.ebcc_hip_reduce_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.POINTER(B.TimeStats)]
    lib.ebcc_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ebcc_hip_timing_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]

    def timed(call):
        assert call() == 0, lib.ebcc_hip_last_error()                     # (warm-up)
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rc = call()
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
            assert rc == 0, lib.ebcc_hip_last_error()
        return ms

    def events(call, name):
        total, launches = ctypes.c_double(), ctypes.c_long()
        lib.ebcc_hip_timing_enable(ctx.ptr, 1)
        lib.ebcc_hip_timing_read(ctx.ptr, name, ctypes.byref(total), ctypes.byref(launches))
        before = total.value
        for _ in range(args.reps):
            assert call() == 0
        lib.ebcc_hip_timing_read(ctx.ptr, name, ctypes.byref(total), ctypes.byref(launches))
        lib.ebcc_hip_timing_enable(ctx.ptr, 0)
        return (total.value - before) / args.reps

    res = {}
    count = np.zeros(4, np.uint64)
    plain = [[torch.empty((H, W), dtype=torch.float64, device=dev) for _ in range(2)] for _ in range(2)]
    st = [B.TimeStats(1, H, W, s.data_ptr(), s2.data_ptr(), None, None, None, 0.0, count.ctypes.data) for s, s2 in plain]

    def two_reduces():
        return (lib.ebcc_hip_reduce_shard(ctx.ptr, var[0][0], var[0][1], N, None, 0, 0, ctypes.byref(st[0])) or
                lib.ebcc_hip_reduce_shard(ctx.ptr, var[1][0], var[1][1], N, None, 0, 0, ctypes.byref(st[1])))

    res["reduce2_ms"] = timed(two_reduces)
    res["reduce2_kernel_ms"] = events(two_reduces, b"time_fold")
    if not args.parent:
        lib.ebcc_hip_pair_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(B.PairStats)]
        lib.ebcc_hip_pair_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(B.PairStats)]
        d = [torch.empty((H, W), dtype=torch.float64, device=dev) for _ in range(6)]
        mx, ov = torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.int32, device=dev)
        p = [t.data_ptr() for t in d]
        sets = {"moments": B.PairStats(1, H, W, p[0], p[1], p[2], p[3], p[4], None, None, None, 0.0, count.ctypes.data),
                "magnitude": B.PairStats(1, H, W, None, None, None, None, None, p[5], mx.data_ptr(), ov.data_ptr(), 15.0, count.ctypes.data),
                "all": B.PairStats(1, H, W, p[0], p[1], p[2], p[3], p[4], p[5], mx.data_ptr(), ov.data_ptr(), 15.0, count.ctypes.data)}
        for key, ps in sets.items():
            call = lambda: lib.ebcc_hip_pair_shard(ctx.ptr, var[0][0], var[0][1], var[1][0], var[1][1], N, None, 0, 0, ctypes.byref(ps))  # noqa: E731
            res[f"pair_{key}_ms"] = timed(call)
            res[f"pair_{key}_kernel_ms"] = events(call, b"pair_fold")
        # the bytes: one call of each into accumulators set anew
        assert lib.ebcc_hip_time_stats_init(ctx.ptr, ctypes.byref(st[0])) == 0 and lib.ebcc_hip_time_stats_init(ctx.ptr, ctypes.byref(st[1])) == 0
        assert lib.ebcc_hip_pair_stats_init(ctx.ptr, ctypes.byref(sets["moments"])) == 0
        assert two_reduces() == 0 and lib.ebcc_hip_pair_shard(ctx.ptr, var[0][0], var[0][1], var[1][0], var[1][1], N, None, 0, 0, ctypes.byref(sets["moments"])) == 0
        for got, want in ((d[0], plain[0][0]), (d[2], plain[0][1]), (d[1], plain[1][0]), (d[3], plain[1][1])):
            assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "the pair decode and the reduce decode disagree"
    for outs, _ in var:
        for i in range(N):
            lib.free_buffer(outs[i])
    ctx.close()
    print("PAIR_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PAIR_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    return json.loads(line[0].split(" ", 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: its two reduce decodes are the yardstick")
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
            print(f"round {rnd} [parent]     y two reduce_shard calls, d_sum + d_sum_sq: {med(a['reduce2_ms']):8.2f} ms {a['reduce2_ms']}; "
                  f"k time_fold {a['reduce2_kernel_ms']:.3f} ms", flush=True)
        b = run_child(common)
        print(f"round {rnd} [this build] y two reduce_shard calls, d_sum + d_sum_sq: {med(b['reduce2_ms']):8.2f} ms {b['reduce2_ms']}; "
              f"k time_fold {b['reduce2_kernel_ms']:.3f} ms", flush=True)
        y = a if a is not None else b
        for row, key, what in ROWS:
            print(f"round {rnd} [this build] {row} pair_shard, {what}: {med(b[f'pair_{key}_ms']):8.2f} ms {b[f'pair_{key}_ms']} "
                  f"= x {med(b[f'pair_{key}_ms']) / med(y['reduce2_ms']):.3f} of {'the parent' if a is not None else 'this build'}'s row y; "
                  f"k pair_fold {b[f'pair_{key}_kernel_ms']:.3f} ms = x {b[f'pair_{key}_kernel_ms'] / y['reduce2_kernel_ms']:.2f} of its time_fold", flush=True)


if __name__ == "__main__":
    main()
