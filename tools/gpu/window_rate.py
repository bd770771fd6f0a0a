"""GPU box: what a window decode costs next to the full decode.  The bench workload - 256 frames
721x1440, base_cr 30, MAX_ERROR 0.5, seeded as bench.py seeds them - is decoded whole and as windows of 360x720, 128x256
(centred and at a corner) and 32x32, device-resident (ebcc_hip_decode_frames[_window]) and into a pageable host array
(ebcc_hip_decode_host_frames[_window]): ms per call, the t1_decode span (ebcc_hip_timing_read), and the share of code-blocks
and of segment bytes each window keeps.

    python tools/gpu/window_rate.py [--rounds 3] [--reps 5] [--parent-lib PATH]

Every measurement is a child process under its own time limit, and nothing more is started after one fails.  With
--parent-lib (the library of the parent commit, built elsewhere) a child that times that library's ebcc_hip_decode_frames
alternates with the children of this build, as tools/gpu/ab_multi.sh alternates settings on one box."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = [("full", None), ("360x720", (180, 360, 360, 720)), ("128x256 centre", (296, 592, 128, 256)), ("128x256 corner", (0, 0, 128, 256)),
         ("32x32", (344, 704, 32, 32))]
CHILD_LIMIT = 420           # seconds for one child (engine set-up, 256 frames coded once, every case a few times)


def child(args):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from tests import _lib as L
    if args.lib:
        L.PRODUCT_SO = args.lib
    lib = L.product()
    H, W, n = bench.H, bench.W, args.frames
    lib.ebcc_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ebcc_hip_timing_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
    lib.ebcc_hip_prepare.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.ebcc_hip_decode_host_frames.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p]
    sig = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t] + [ctypes.c_size_t] * 4 + [ctypes.c_void_p]
    if not args.full_only:
        lib.ebcc_hip_decode_frames_window.argtypes = sig
        lib.ebcc_hip_decode_host_frames_window.argtypes = sig
        lib.ebcc_hip_window_plan.argtypes = [ctypes.c_size_t] * 6 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    device = torch.device("cuda", 0)
    ctx = lib.ebcc_hip_create(0, n, H, W)
    assert ctx, lib.ebcc_hip_last_error()
    assert lib.ebcc_hip_prepare(ctx, n) == 0
    frames = bench.synth_frames(torch, n, device, seed=0)
    torch.cuda.synchronize()
    cfg = L.make_config((1, H, W), base_cr=bench.BASE_CR, error=bench.MAX_ERR, residual_type=L.MAX_ERROR)
    outs, sizes = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)()
    assert lib.ebcc_hip_encode_frames(ctx, frames.data_ptr(), n, ctypes.byref(cfg), outs, sizes) == 0, lib.ebcc_hip_last_error()
    d_out = torch.empty_like(frames)
    res = {}
    for name, win in CASES if not args.full_only else CASES[:1]:
        pix = H * W if win is None else win[2] * win[3]

        def resident():
            rc = (lib.ebcc_hip_decode_frames(ctx, outs, sizes, n, d_out.data_ptr()) if win is None else
                  lib.ebcc_hip_decode_frames_window(ctx, outs, sizes, n, *win, d_out.data_ptr()))
            assert rc == 0, lib.ebcc_hip_last_error()

        def host():
            h_out = np.empty(n * pix, np.float32)                      # (a fresh pageable array every call, as a reader has)
            t0 = time.perf_counter()
            rc = (lib.ebcc_hip_decode_host_frames(ctx, outs, sizes, n, h_out.ctypes.data) if win is None else
                  lib.ebcc_hip_decode_host_frames_window(ctx, outs, sizes, n, *win, h_out.ctypes.data))
            assert rc == 0, lib.ebcc_hip_last_error()
            return time.perf_counter() - t0

        r = {}
        resident()                                                      # (warm-up)
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            resident()
            t.append(time.perf_counter() - t0)
        r["resident_ms"] = [round(1e3 * v, 3) for v in t]
        lib.ebcc_hip_timing_enable(ctx, 1)
        resident()
        a, c = ctypes.c_double(), ctypes.c_long()
        lib.ebcc_hip_timing_read(ctx, b"t1_decode", ctypes.byref(a), ctypes.byref(c))
        lib.ebcc_hip_timing_enable(ctx, 0)
        r["t1_decode_ms"], r["t1_decode_spans"] = round(a.value, 3), c.value
        host()
        r["host_ms"] = [round(1e3 * host(), 3) for _ in range(args.reps)]
        if not args.full_only:
            if win is None:
                r["blocks_kept"], r["blocks"] = 298, 298
            else:
                blocks = np.zeros((512, 6), np.int32)
                bands = np.zeros((16, 4), np.int32)
                nb = lib.ebcc_hip_window_plan(H, W, *win, bands.ctypes.data, blocks.ctypes.data, 512)
                r["blocks_kept"], r["blocks"] = int(blocks[:nb, 5].sum()), nb
            os.environ["EBCC_HIP_T1_STATS"] = "1"                      # (the decoder reports the bytes of the segments it was given, on stderr)
            print(f"WINDOW_STATS_BEGIN {name}", file=sys.stderr, flush=True)
            resident()
            print("WINDOW_STATS_END", file=sys.stderr, flush=True)
            del os.environ["EBCC_HIP_T1_STATS"]
        res[name] = r
    res["stream_bytes"] = int(sum(sizes[i] for i in range(n)))
    for i in range(n):
        lib.free_buffer(outs[i])
    lib.ebcc_hip_destroy(ctx)
    print("WINDOW_RATE " + json.dumps(res), flush=True)


def run_child(extra, frames, reps):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", "--frames", str(frames), "--reps", str(reps)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("WINDOW_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra) or '(this build)'} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    res = json.loads(line[0].split(" ", 1)[1])
    # segment bytes per case: the sum over the slices' "t1 decode: N code-blocks, B bytes" lines between the markers
    name = None
    for ln in r.stderr.splitlines():
        if ln.startswith("WINDOW_STATS_BEGIN "):
            name = ln.split(" ", 1)[1]
            res[name]["segment_bytes"] = 0
        elif ln.startswith("WINDOW_STATS_END"):
            name = None
        elif name:
            m = re.search(r"t1 decode: \d+ code-blocks, (\d+) bytes", ln)
            if m:
                res[name]["segment_bytes"] += int(m.group(1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: its full decode is timed in alternation")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--full-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    def med(v):
        return sorted(v)[len(v) // 2]

    for rnd in range(args.rounds):
        if args.parent_lib:
            p = run_child(["--lib", os.path.abspath(args.parent_lib), "--full-only"], args.frames, args.reps)["full"]
            print(f"round {rnd} [parent] full decode: resident {med(p['resident_ms']):8.2f} ms (min {min(p['resident_ms']):.2f}), t1_decode {p['t1_decode_ms']:.2f} ms, "
                  f"host array {med(p['host_ms']):8.2f} ms (min {min(p['host_ms']):.2f})", flush=True)
        res = run_child([], args.frames, args.reps)
        full_bytes = res["full"].get("segment_bytes", 0)
        for name, _ in CASES:
            r = res[name]
            share = f"{100.0 * r['segment_bytes'] / full_bytes:5.1f} %" if full_bytes else "    ?"
            print(f"round {rnd} [this build] {name:15s}: resident {med(r['resident_ms']):8.2f} ms (min {min(r['resident_ms']):.2f}), t1_decode {r['t1_decode_ms']:6.2f} ms in "
                  f"{r['t1_decode_spans']} spans, host array {med(r['host_ms']):8.2f} ms (min {min(r['host_ms']):.2f}); code-blocks kept {r['blocks_kept']}/{r['blocks']}, "
                  f"segment bytes {r.get('segment_bytes', 0)} ({share})", flush=True)


if __name__ == "__main__":
    main()
