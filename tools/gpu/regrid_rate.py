"""GPU box: what the regrid decode costs on the bench workload ("Regrid decode").
256 frames of 721x1440 from the bench's field generator, coded with base_cr 30 and MAX_ERROR 0.5 and resident as streams, a
context of 256 frames.
  1  ebcc_hip_decode_shard into [256][H][W] on the device: the parent's library (--parent-lib) and this build - the yardstick;
     beside it, from both, ebcc_hip_decode_host_frames and ebcc_hip_decode_shard_window of the regional box
  2  ebcc_hip_regrid_shard with the conservative 721x1440 -> 181x360 map (sin(latitude) rows, periodic columns)
  3  the same through ebcc_hip_regrid_host_frames, against the parent's ebcc_hip_decode_host_frames
  4  a regional map: 4 x 4 block means of a 200 x 300 box -> 50 x 75 (decoded as a window)
  5  the kernel's launches alone (ebcc_hip_regrid_items on the decoded frames, timed with events: ebcc_hip_timing_read
     "regrid"), in GB/s of the frames read
ms are the median of --reps calls after one warm-up.  Every run asserts that rows 2 to 4 are, byte for byte,
ebcc_hip_regrid_items of what ebcc_hip_decode_shard gave.  The lines, set against the parent of the same round:
  row 2 not above the parent's row 1 plus twice the kernel pass of row 5;
  row 3 below the parent's host decode by more than the spread (max - min) of the parent's calls of that round;
  row 4 not above the parent's window decode of that box plus twice the kernel pass of row 5.

    python tools/gpu/regrid_rate.py [--parent-lib PATH] [--rounds 2] [--reps 5]

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
    lib.ebcc_hip_decode_host_frames.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.ebcc_hip_decode_shard_window.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t] + [ctypes.c_size_t] * 4 + [ctypes.c_void_p]

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
    win = torch.empty((N, BOX[2], BOX[3]), dtype=torch.float32, device=frames.device)
    res["window_ms"] = timed(lambda: lib.ebcc_hip_decode_shard_window(ctx.ptr, outs, sizes, N, *BOX, win.data_ptr()))
    host = np.empty((N, H, W), np.float32)
    res["host_decode_ms"] = timed(lambda: lib.ebcc_hip_decode_host_frames(ctx.ptr, outs, sizes, N, host.ctypes.data))
    del host
    if not args.parent:
        from ebcc_amd import regrid as M
        lib.ebcc_hip_regrid_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.POINTER(M.RegridSpec), ctypes.c_void_p]
        for name in ("ebcc_hip_regrid_shard", "ebcc_hip_regrid_host_frames"):
            getattr(lib, name).argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.POINTER(M.RegridSpec), ctypes.c_void_p]
        lib.ebcc_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.ebcc_hip_timing_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
        lat1, lon1 = np.linspace(90.0, -90.0, 181), np.arange(360) * 1.0
        world = (M.conservative_map(M.cell_edges(lat, -90, 90), M.cell_edges(lat1, -90, 90), measure=lambda e: np.sin(np.deg2rad(e))),
                 M.conservative_map(M.cell_edges(lon), M.cell_edges(lon1), period=360.0))
        rows, cols = M.block_mean_map(BOX[2], 4), M.block_mean_map(BOX[3], 4)
        region = (M.AxisMap(rows.first.astype(np.int64) + BOX[0], rows.count, rows.weight), M.AxisMap(cols.first.astype(np.int64) + BOX[1], cols.count, cols.weight))

        def events(call):
            lib.ebcc_hip_timing_enable(ctx.ptr, 1)
            for _ in range(args.reps):
                assert call() == 0
            total, launches = ctypes.c_double(), ctypes.c_long()
            lib.ebcc_hip_timing_read(ctx.ptr, b"regrid", ctypes.byref(total), ctypes.byref(launches))
            lib.ebcc_hip_timing_enable(ctx.ptr, 0)
            return total.value / max(1, launches.value)

        frame_bytes = N * H * W * 4
        for key, (rm, cm) in (("world", world), ("region", region)):
            spec = M.regrid_spec(rm, cm)
            shape = (N, rm.n_out, cm.n_out)
            got = torch.empty(shape, dtype=torch.float32, device=frames.device)
            ref = torch.empty(shape, dtype=torch.float32, device=frames.device)
            res[f"regrid_{key}_ms"] = timed(lambda: lib.ebcc_hip_regrid_shard(ctx.ptr, outs, sizes, N, ctypes.byref(spec), got.data_ptr()))
            items = lambda: lib.ebcc_hip_regrid_items(ctx.ptr, dec.data_ptr(), N, H, W, ctypes.byref(spec), ref.data_ptr())  # noqa: E731
            res[f"items_{key}_call_ms"] = timed(items)
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{key}: the regrid decode and the kernel on the decoded frames disagree"
            if key == "world":
                h_out = np.empty(shape, np.float32)
                res["regrid_host_ms"] = timed(lambda: lib.ebcc_hip_regrid_host_frames(ctx.ptr, outs, sizes, N, ctypes.byref(spec), h_out.ctypes.data))
                assert h_out.tobytes() == ref.cpu().numpy().tobytes(), "the host form and the kernel on the decoded frames disagree"
            ms = events(items)
            res[f"items_{key}_event_ms"] = ms
            res[f"items_{key}_gb_s"] = (frame_bytes if key == "world" else N * BOX[2] * BOX[3] * 4) / (ms * 1e-3) / 1e9
    for i in range(N):
        lib.free_buffer(outs[i])
    ctx.close()
    print("REGRID_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("REGRID_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    return json.loads(line[0].split(" ", 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: its decodes are the yardstick")
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
            print(f"round {rnd} [parent]     decode_shard {med(a['decode_ms']):8.2f} ms {a['decode_ms']}; decode_shard_window of the box {med(a['window_ms']):.2f} ms; "
                  f"decode_host_frames {med(a['host_decode_ms']):.2f} ms {a['host_decode_ms']}", flush=True)
        b = run_child(common)
        print(f"round {rnd} [this build] decode_shard {med(b['decode_ms']):8.2f} ms {b['decode_ms']}; decode_shard_window of the box {med(b['window_ms']):.2f} ms; "
              f"decode_host_frames {med(b['host_decode_ms']):.2f} ms; regrid_shard 181 x 360 {med(b['regrid_world_ms']):.2f} ms {b['regrid_world_ms']}; "
              f"regrid_host_frames {med(b['regrid_host_ms']):.2f} ms {b['regrid_host_ms']}; regrid_shard of the box {med(b['regrid_region_ms']):.2f} ms; "
              f"regrid_items call: world {med(b['items_world_call_ms']):.2f} ms, box {med(b['items_region_call_ms']):.2f} ms; its launches alone: world "
              f"{b['items_world_event_ms']:.3f} ms = {b['items_world_gb_s']:.0f} GB/s of frames, box {b['items_region_event_ms']:.3f} ms = "
              f"{b['items_region_gb_s']:.0f} GB/s of the box", flush=True)
        if a is not None:
            allow = 2 * b["items_world_event_ms"]
            line2 = med(a["decode_ms"]) + allow
            spread = max(a["host_decode_ms"]) - min(a["host_decode_ms"])
            line3 = med(a["host_decode_ms"]) - spread
            line4 = med(a["window_ms"]) + allow
            verdict = lambda ok: "within" if ok else "MISSED"                # noqa: E731
            print(f"round {rnd} line 2: parent decode + 2 x the kernel pass = {line2:.2f} ms; regrid_shard {med(b['regrid_world_ms']):.2f} ms: "
                  f"{verdict(med(b['regrid_world_ms']) <= line2)}", flush=True)
            print(f"round {rnd} line 3: parent host decode - its spread ({spread:.2f}) = {line3:.2f} ms; regrid_host_frames {med(b['regrid_host_ms']):.2f} ms: "
                  f"{verdict(med(b['regrid_host_ms']) < line3)}", flush=True)
            print(f"round {rnd} line 4: parent window decode + 2 x the kernel pass = {line4:.2f} ms; regrid_shard of the box {med(b['regrid_region_ms']):.2f} ms: "
                  f"{verdict(med(b['regrid_region_ms']) <= line4)}", flush=True)


if __name__ == "__main__":
    main()
