"""GPU box: what the area series costs on the bench workload ("Area series").
256 frames of 721x1440 from the bench's field generator, coded with base_cr 30 and MAX_ERROR 0.5 and resident as streams, a
context of 256 frames.
  1  ebcc_hip_decode_shard into [256][H][W] on the device: the parent's library (--parent-lib) and this build - the yardstick
  2  ebcc_hip_series_shard, one whole-frame region with cos(latitude) row weights
  3  the same with 721 one-row regions (zonal means)
  4  the same with one 200 x 300 region (decoded as a window)
  5  the launches of the fold alone (ebcc_hip_area_fold on the decoded frames, timed with events: ebcc_hip_timing_read
     "area_fold"), one region and 721, in GB/s of frames read; beside it the audit's statistics pass over the same frames
     (ebcc_hip_frame_errors, "frame_errors"), which reads two arrays
ms are the median of --reps calls after one warm-up.  Every run asserts that the records of row 2 are, byte for byte, the fold
of what ebcc_hip_decode_shard gave.  The line set for row 2: not above the parent's decode of the same round plus twice the
statistics pass.

    python tools/gpu/series_rate.py [--parent-lib PATH] [--rounds 2] [--reps 5]

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


def med(v):
    return sorted(v)[len(v) // 2]


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from tests import _lib as L
    from tests import _series as S
    if args.lib:
        L.PRODUCT_SO = args.lib
    lib = L.product()
    import bench
    H, W = bench.H, bench.W
    frames = bench.synth_frames(torch, N, torch.device("cuda", 0), seed=0)
    torch.cuda.synchronize()
    ctx = L.Context(N, H, W)
    lib.ebcc_hip_prepare.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert lib.ebcc_hip_prepare(ctx.ptr, N) == 0
    cfg = L.make_config((1, H, W), base_cr=bench.BASE_CR, error=bench.MAX_ERR, residual_type=L.MAX_ERROR)
    outs, sizes = (ctypes.c_void_p * N)(), (ctypes.c_size_t * N)()
    assert lib.ebcc_hip_encode_shard(ctx.ptr, frames.data_ptr(), N, ctypes.byref(cfg), outs, sizes) == 0, lib.ebcc_hip_last_error()

    def timed(call):
        assert call() == 0, lib.ebcc_hip_last_error()                     # (warm-up)
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rc = call()
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
            assert rc == 0, lib.ebcc_hip_last_error()
        return ms

    dec = torch.empty_like(frames)
    res = {"decode_ms": timed(lambda: lib.ebcc_hip_decode_shard(ctx.ptr, outs, sizes, N, dec.data_ptr()))}
    if not args.parent:
        lib.ebcc_hip_area_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(S.AreaSpec),
                                           ctypes.c_void_p]
        lib.ebcc_hip_series_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.POINTER(S.AreaSpec), ctypes.c_void_p]
        lib.ebcc_hip_frame_errors.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_void_p]
        lib.ebcc_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.ebcc_hip_timing_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        w_row = np.cos(np.deg2rad(np.linspace(90.0, -90.0, H)))
        w_row[0] = w_row[-1] = 0.0                                        # (the poles: cos gives 6e-17)

        def events(name, call):
            lib.ebcc_hip_timing_enable(ctx.ptr, 1)
            for _ in range(args.reps):
                assert call() == 0
            total, launches = ctypes.c_double(), ctypes.c_long()
            lib.ebcc_hip_timing_read(ctx.ptr, name, ctypes.byref(total), ctypes.byref(launches))
            lib.ebcc_hip_timing_enable(ctx.ptr, 0)
            return total.value / max(1, launches.value)

        frame_bytes = N * H * W * 4
        lists = {"whole": [(0, 0, H, W)], "zonal": [(r, 0, 1, W) for r in range(H)], "box": [BOX]}
        for key, regions in lists.items():
            table = S.region_array(regions)
            spec = S.AreaSpec(len(regions), ctypes.addressof(table), w_row.ctypes.data, None, 1, 280.0)
            got, folded = np.zeros((N, len(regions)), S.AREA_STAT), np.zeros((N, len(regions)), S.AREA_STAT)
            res[f"series_{key}_ms"] = timed(lambda: lib.ebcc_hip_series_shard(ctx.ptr, outs, sizes, N, ctypes.byref(spec), got.ctypes.data))
            fold = lambda: lib.ebcc_hip_area_fold(ctx.ptr, dec.data_ptr(), N, H, W, ctypes.byref(spec), folded.ctypes.data)  # noqa: E731
            res[f"fold_{key}_call_ms"] = timed(fold)
            assert got.tobytes() == folded.tobytes(), f"{key}: the series and the fold of the decoded frames disagree"
            if key != "box":
                ms = events(b"area_fold", fold)
                res[f"fold_{key}_event_ms"] = ms
                res[f"fold_{key}_gb_s"] = frame_bytes / (ms * 1e-3) / 1e9
        report = np.zeros(N, [("max_abs", "<f4"), ("at", "<u4"), ("n_over", "<u8"), ("sum", "<f8"), ("sum_sq", "<f8"), ("x_min", "<f4"), ("x_max", "<f4")])
        stats = lambda: lib.ebcc_hip_frame_errors(ctx.ptr, frames.data_ptr(), dec.data_ptr(), N, H, W, None, report.ctypes.data)  # noqa: E731
        res["stats_call_ms"] = timed(stats)
        ms = events(b"frame_errors", stats)
        res["stats_event_ms"] = ms
        res["stats_gb_s"] = 2 * frame_bytes / (ms * 1e-3) / 1e9
    for i in range(N):
        lib.free_buffer(outs[i])
    ctx.close()
    print("SERIES_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SERIES_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    return json.loads(line[0].split(" ", 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: its ebcc_hip_decode_shard is the yardstick")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--parent", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    common = ["--reps", str(args.reps)]
    for rnd in range(args.rounds):
        yard = None
        if args.parent_lib:
            a = run_child(common + ["--parent", "--lib", os.path.abspath(args.parent_lib)])
            yard = med(a["decode_ms"])
            print(f"round {rnd} [parent]     decode_shard {yard:8.2f} ms", flush=True)
        b = run_child(common)
        print(f"round {rnd} [this build] decode_shard {med(b['decode_ms']):8.2f} ms; series_shard: one whole-frame region {med(b['series_whole_ms']):.2f} ms, "
              f"721 one-row regions {med(b['series_zonal_ms']):.2f} ms, one {BOX[2]} x {BOX[3]} region {med(b['series_box_ms']):.2f} ms; "
              f"area_fold call: one region {med(b['fold_whole_call_ms']):.2f} ms, 721 regions {med(b['fold_zonal_call_ms']):.2f} ms; its launches alone: "
              f"one region {b['fold_whole_event_ms']:.3f} ms = {b['fold_whole_gb_s']:.0f} GB/s of frames, 721 regions {b['fold_zonal_event_ms']:.3f} ms = "
              f"{b['fold_zonal_gb_s']:.0f} GB/s; frame_errors call {med(b['stats_call_ms']):.2f} ms, its launches {b['stats_event_ms']:.3f} ms = "
              f"{b['stats_gb_s']:.0f} GB/s over two arrays", flush=True)
        if yard is not None:
            line = yard + 2 * b["stats_event_ms"]
            print(f"round {rnd} the line: parent decode + 2 x the statistics pass' launches = {line:.2f} ms; one whole-frame region {med(b['series_whole_ms']):.2f} ms: "
                  f"{'within' if med(b['series_whole_ms']) <= line else 'ABOVE'}", flush=True)


if __name__ == "__main__":
    main()
