"""GPU box: what the audit and the hard error bound cost on the bench workload ("Hard bound").
256 frames of 721x1440 from the bench's field generator, resident on the device, base_cr 30, a context of 256 frames.
  audit  ebcc_hip_audit_frames of the plain call's streams against ebcc_hip_decode_frames of the same streams (this build, and the
         parent's library where --parent-lib is given), and the two statistics launches alone (ebcc_hip_frame_errors on the
         frames and their decode, timed with events: ebcc_hip_timing_read "frame_errors") with the HBM rate they reach
  hard   ebcc_hip_encode_shard_hard against ebcc_hip_encode_shard (this build and the parent's library), for MAX_ERROR 0.5 and
         RELATIVE_ERROR 1e-3: ms per call, the share of the frames coded again in each round, the rounds histogram, the growth
         in bytes, and the largest achieved / target before (the audit of the plain streams) and after
ms are the median of --reps calls after one warm-up.

    python tools/gpu/hard_rate.py [--parent-lib PATH] [--rounds 1] [--reps 5]

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
MODES = {"MAX_ERROR": 0.5, "RELATIVE_ERROR": 1e-3}
FRAME_ERROR = [("max_abs", "<f4"), ("at", "<u4"), ("n_over", "<u8"), ("sum", "<f8"), ("sum_sq", "<f8"), ("x_min", "<f4"), ("x_max", "<f4")]
BOUND_REPORT = [("target", "<f4"), ("achieved", "<f4"), ("error_used", "<f4"), ("rounds", "<i4"), ("met", "<i4")]


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
    H, W = bench.H, bench.W
    frames = bench.synth_frames(torch, N, torch.device("cuda", 0), seed=0)
    torch.cuda.synchronize()
    ctx = L.Context(N, H, W)
    lib.ebcc_hip_prepare.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert lib.ebcc_hip_prepare(ctx.ptr, N) == 0
    cfg = L.make_config((1, H, W), base_cr=bench.BASE_CR, error=MODES[args.mode], residual_type=getattr(L, args.mode))
    outs, sizes = (ctypes.c_void_p * N)(), (ctypes.c_size_t * N)()

    def release():
        total = sum(sizes[i] for i in range(N))
        for i in range(N):
            lib.free_buffer(outs[i])
        return total

    def timed(call, after=lambda: None):
        call()                                                           # (warm-up)
        after()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
            after()
        return ms

    def plain():
        assert lib.ebcc_hip_encode_shard(ctx.ptr, frames.data_ptr(), N, ctypes.byref(cfg), outs, sizes) == 0, lib.ebcc_hip_last_error()

    res = {}
    if args.parent:
        if args.what == "hard":
            res["plain_ms"] = timed(plain, release)
        else:
            plain()
            dec = torch.empty_like(frames)
            res["decode_ms"] = timed(lambda: lib.ebcc_hip_decode_frames(ctx.ptr, outs, sizes, N, dec.data_ptr()))
            release()
    elif args.what == "audit":
        audit = lib.ebcc_hip_audit_frames
        audit.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.ebcc_hip_frame_errors.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_void_p]
        lib.ebcc_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.ebcc_hip_timing_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        plain()
        dec = torch.empty_like(frames)
        report = np.zeros(N, FRAME_ERROR)
        bound = np.full(N, MODES[args.mode], np.float32)
        res["decode_ms"] = timed(lambda: lib.ebcc_hip_decode_frames(ctx.ptr, outs, sizes, N, dec.data_ptr()))
        res["audit_ms"] = timed(lambda: audit(ctx.ptr, outs, sizes, N, frames.data_ptr(), bound.ctypes.data, report.ctypes.data))
        alone = np.zeros(N, FRAME_ERROR)
        res["stats_call_ms"] = timed(lambda: lib.ebcc_hip_frame_errors(ctx.ptr, frames.data_ptr(), dec.data_ptr(), N, H, W, bound.ctypes.data, alone.ctypes.data))
        assert alone.tobytes() == report.tobytes(), "the audit and the kernel alone disagree"
        lib.ebcc_hip_timing_enable(ctx.ptr, 1)
        for _ in range(args.reps):
            lib.ebcc_hip_frame_errors(ctx.ptr, frames.data_ptr(), dec.data_ptr(), N, H, W, bound.ctypes.data, alone.ctypes.data)
        total, launches = ctypes.c_double(), ctypes.c_long()
        lib.ebcc_hip_timing_read(ctx.ptr, b"frame_errors", ctypes.byref(total), ctypes.byref(launches))
        lib.ebcc_hip_timing_enable(ctx.ptr, 0)
        res["stats_event_ms"] = total.value / max(1, launches.value)
        res["stats_tb_s"] = 2 * N * H * W * 4 / (res["stats_event_ms"] * 1e-3) / 1e12
        res["over"] = int((report["n_over"] > 0).sum())
        release()
    else:
        hard = lib.ebcc_hip_encode_shard_hard
        hard.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(L.CodecConfig), ctypes.c_int, L.c_void_pp, L.c_size_p,
                         ctypes.c_void_p]
        audit = lib.ebcc_hip_audit_frames
        audit.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        report = np.zeros(N, BOUND_REPORT)
        before = np.zeros(N, FRAME_ERROR)
        plain()
        assert audit(ctx.ptr, outs, sizes, N, frames.data_ptr(), None, before.ctypes.data) == 0
        res["plain_bytes"] = release()
        res["plain_ms"] = timed(plain, release)
        status = []
        res["hard_ms"] = timed(lambda: status.append(hard(ctx.ptr, frames.data_ptr(), N, ctypes.byref(cfg), 0, outs, sizes, report.ctypes.data)),
                               lambda: res.__setitem__("hard_bytes", release()))
        assert set(status) <= {0, 3}, status
        res["status"] = status[-1]
        res["rounds_hist"] = np.bincount(report["rounds"]).tolist()
        res["share_per_round"] = [round(float((report["rounds"] >= k).mean()), 4) for k in range(1, int(report["rounds"].max()) + 1)]
        res["worst_before"] = float((before["max_abs"] / report["target"]).max())
        res["worst_after"] = float((report["achieved"] / report["target"]).max())
        res["not_met"] = int((report["met"] == 0).sum())
    ctx.close()
    print("HARD_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("HARD_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    return json.loads(line[0].split(" ", 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: its ebcc_hip_decode_frames / ebcc_hip_encode_shard are the yardsticks")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--parent", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--what", default="audit", help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="MAX_ERROR", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    common = ["--reps", str(args.reps)]
    parent = ["--parent", "--lib", os.path.abspath(args.parent_lib)] if args.parent_lib else None
    for rnd in range(args.rounds):
        if parent:
            a = run_child(common + parent + ["--what", "audit"])
            print(f"round {rnd} audit [parent]     decode_frames {med(a['decode_ms']):8.2f} ms", flush=True)
        b = run_child(common + ["--what", "audit"])
        print(f"round {rnd} audit [this build] decode_frames {med(b['decode_ms']):8.2f} ms, audit_frames {med(b['audit_ms']):8.2f} ms, "
              f"frame_errors call {med(b['stats_call_ms']):.2f} ms, its two launches {b['stats_event_ms']:.3f} ms = {b['stats_tb_s']:.2f} TB/s; "
              f"{b['over']} of {N} frames over MAX_ERROR 0.5", flush=True)
        for mode in MODES:
            if parent:
                a = run_child(common + parent + ["--what", "hard", "--mode", mode])
                print(f"round {rnd} {mode} [parent]     encode_shard {med(a['plain_ms']):8.2f} ms", flush=True)
            b = run_child(common + ["--what", "hard", "--mode", mode])
            print(f"round {rnd} {mode} [this build] encode_shard {med(b['plain_ms']):8.2f} ms, encode_shard_hard {med(b['hard_ms']):8.2f} ms (status {b['status']}, "
                  f"{b['not_met']} not met); share coded again per round {b['share_per_round']}, rounds histogram {b['rounds_hist']}; bytes "
                  f"{b['plain_bytes']} -> {b['hard_bytes']} ({100.0 * (b['hard_bytes'] / b['plain_bytes'] - 1):+.2f}%); worst achieved / target "
                  f"{b['worst_before']:.4f} -> {b['worst_after']:.4f}", flush=True)


if __name__ == "__main__":
    main()
