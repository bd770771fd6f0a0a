"""GPU box: what the time-map decode costs on the bench workload ("Time-map decode").
256 frames of 721x1440 from the bench's field generator, coded with base_cr 30 and MAX_ERROR 0.5 and resident as streams, a
context of 256 frames.
  y  ebcc_hip_reduce_shard with one bin and d_sum only, the parent's library (--parent-lib) and this build - the yardstick: one
     decode plus one streaming pass over the decoded batch; for whole frames and for the 200 x 300 box at (260, 570)
  1  ebcc_hip_project_shard, one output naming every frame (the yardstick's work plus a multiply), whole frames and the box
  2  2 outputs, the trend map (h5_batch.trend_weights), whole frames
  3  16 dense outputs (harmonics-like cosine / sine weights): four groups of four
  4  the same 16 outputs, output o without its term of frame o: no two neighbours name the same frames, no group forms
  5  a running mean of width 5 (252 outputs) on the box
  6  the kernel alone (ebcc_hip_time_map_items on the decoded frames, timed with events: ebcc_hip_timing_read "time_map") for
     the maps of rows 1 to 5, per call, with the GB/s of the items its entries read
ms are the median of --reps calls after one warm-up.  Every run asserts that rows 1 to 5 are, byte for byte,
ebcc_hip_time_map_items of what ebcc_hip_decode_shard gave.

    python tools/gpu/time_map_rate.py [--parent-lib PATH] [--rounds 2] [--reps 5]

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
ROWS = (("1", "one", "one output, whole frames"), ("1", "one_box", "one output, the box"), ("2", "trend", "the trend map, whole frames"),
        ("3", "dense16", "16 dense outputs, groups"), ("4", "apart16", "16 outputs, no group"), ("5", "running", "running mean of 5, 252 outputs, the box"))


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
    count = np.zeros(256, np.uint64)
    for key, (row0, col0, rows, cols) in (("whole", (0, 0, H, W)), ("box", BOX)):
        s = torch.empty((rows, cols), dtype=torch.float64, device=dev)
        st = B.TimeStats(1, rows, cols, s.data_ptr(), None, None, None, None, 0.0, count.ctypes.data)
        assert lib.ebcc_hip_time_stats_init(ctx.ptr, ctypes.byref(st)) == 0
        res[f"reduce_{key}_ms"] = timed(lambda: lib.ebcc_hip_reduce_shard(ctx.ptr, outs, sizes, N, None, row0, col0, ctypes.byref(st)))
    if not args.parent:
        lib.ebcc_hip_time_map_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(B.TimeMap)]
        lib.ebcc_hip_time_map_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(B.TimeMap)]
        lib.ebcc_hip_project_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                               ctypes.POINTER(B.TimeMap)]
        lib.ebcc_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.ebcc_hip_timing_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        dec = torch.empty_like(frames)
        assert lib.ebcc_hip_decode_shard(ctx.ptr, outs, sizes, N, dec.data_ptr()) == 0, lib.ebcc_hip_last_error()
        del frames

        def events(call):
            lib.ebcc_hip_timing_enable(ctx.ptr, 1)
            for _ in range(args.reps):
                assert call() == 0
            total, launches = ctypes.c_double(), ctypes.c_long()
            lib.ebcc_hip_timing_read(ctx.ptr, b"time_map", ctypes.byref(total), ctypes.byref(launches))
            lib.ebcc_hip_timing_enable(ctx.ptr, 0)
            return total.value / args.reps

        t = np.arange(N, dtype=np.float64)
        angle = 2 * np.pi * (t + 0.5) / N                             # (half a step off: no weight is exactly 0)
        harmonics = np.stack([fn(angle * (k + 1)) for k in range(8) for fn in (np.cos, np.sin)])
        apart = harmonics.copy()
        apart[np.arange(16), np.arange(16)] = 0.0
        assert (harmonics != 0).all() and (B.trend_weights(t) != 0).all()
        # {row: (weights, window, list entries of the one batch: a group of outputs has one entry per item)}
        maps = {"one": (np.full((1, N), 1.0 / 3.0), (0, 0, H, W), N), "one_box": (np.full((1, N), 1.0 / 3.0), BOX, N),
                "trend": (B.trend_weights(t), (0, 0, H, W), N), "dense16": (harmonics, (0, 0, H, W), 4 * N),
                "apart16": (apart, (0, 0, H, W), 16 * (N - 1)), "running": (B.running_mean_weights(N, 5), BOX, 252 * 5)}
        for key, (dense, (row0, col0, rows, cols), entries) in maps.items():
            start, frame, weight = B.time_map_terms(dense)
            n_out = len(start) - 1
            got = torch.empty((n_out, rows, cols), dtype=torch.float64, device=dev)
            ref = torch.empty((n_out, rows, cols), dtype=torch.float64, device=dev)
            m = B.TimeMap(n_out, rows, cols, start.ctypes.data, frame.ctypes.data, weight.ctypes.data, got.data_ptr(), count.ctypes.data)
            r = B.TimeMap(n_out, rows, cols, start.ctypes.data, frame.ctypes.data, weight.ctypes.data, ref.data_ptr(), count.ctypes.data)
            res[f"project_{key}_ms"] = timed(lambda: lib.ebcc_hip_project_shard(ctx.ptr, outs, sizes, N, row0, col0, ctypes.byref(m)))
            crop = dec if (rows, cols) == (H, W) else dec[:, row0:row0 + rows, col0:col0 + cols].contiguous()
            items = lambda: lib.ebcc_hip_time_map_items(ctx.ptr, crop.data_ptr(), N, ctypes.byref(r))  # noqa: E731
            # the bytes: one call of each into accumulators set to 0
            assert lib.ebcc_hip_time_map_init(ctx.ptr, ctypes.byref(m)) == 0 and lib.ebcc_hip_time_map_init(ctx.ptr, ctypes.byref(r)) == 0
            assert lib.ebcc_hip_project_shard(ctx.ptr, outs, sizes, N, row0, col0, ctypes.byref(m)) == 0 and items() == 0
            assert torch.equal(got.view(torch.int64), ref.view(torch.int64)), f"{key}: the time-map decode and the kernel on the decoded frames disagree"
            res[f"items_{key}_call_ms"] = timed(items)
            res[f"items_{key}_kernel_ms"] = events(items)
            res[f"items_{key}_gb_s"] = entries * rows * cols * 4 / (res[f"items_{key}_kernel_ms"] * 1e-3) / 1e9
            del got, ref
    for i in range(N):
        lib.free_buffer(outs[i])
    ctx.close()
    print("TIME_MAP_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TIME_MAP_RATE ")]
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
            print(f"round {rnd} [parent]     y reduce_shard, one bin, d_sum: whole frames {med(a['reduce_whole_ms']):8.2f} ms {a['reduce_whole_ms']}; "
                  f"the box {med(a['reduce_box_ms']):.2f} ms {a['reduce_box_ms']}", flush=True)
        b = run_child(common)
        print(f"round {rnd} [this build] y reduce_shard, one bin, d_sum: whole frames {med(b['reduce_whole_ms']):8.2f} ms {b['reduce_whole_ms']}; "
              f"the box {med(b['reduce_box_ms']):.2f} ms {b['reduce_box_ms']}", flush=True)
        y = a if a is not None else b
        for row, key, what in ROWS:
            base = med(y["reduce_box_ms" if "box" in what else "reduce_whole_ms"])
            print(f"round {rnd} [this build] {row} project_shard, {what}: {med(b[f'project_{key}_ms']):8.2f} ms {b[f'project_{key}_ms']} "
                  f"= x {med(b[f'project_{key}_ms']) / base:.2f} of {'the parent' if a is not None else 'this build'}'s row y", flush=True)
            print(f"round {rnd} [this build] 6 time_map_items on the decoded frames, {what}: call {med(b[f'items_{key}_call_ms']):.2f} ms, kernels "
                  f"{b[f'items_{key}_kernel_ms']:.3f} ms = {b[f'items_{key}_gb_s']:.0f} GB/s of the items read", flush=True)


if __name__ == "__main__":
    main()
