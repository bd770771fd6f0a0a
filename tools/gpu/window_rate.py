"""GPU box: what a window decode costs next to the full decode.  The bench workload - 256 frames
721x1440, base_cr 30, MAX_ERROR 0.5, seeded as bench.py seeds them - is decoded whole and as windows of 360x720, 128x256
(centred and at a corner) and 32x32, device-resident (ebcc_hip_decode_frames[_window]) and into a pageable host array
(ebcc_hip_decode_host_frames[_window]): ms per call, the t1_decode span (ebcc_hip_timing_read), and the share of code-blocks
and of segment bytes each window keeps.  Then the box lists (ebcc_hip_decode_*_boxes), each next to the only way without them:
stations (64 seeded points of every frame in one call, against 64 window calls), a track (a 128x256 box that moves over the 256
frames, against the uniform window of its bounding box), a sparse list (the centred 128x256 box on every eighth frame, against
the same window on those 32 streams), and the four uniform windows as box lists of one box per frame (DESIGN section 2.8:
one path or two).

    python tools/gpu/window_rate.py [--rounds 3] [--reps 5] [--parent-lib PATH]

Every measurement is a child process under its own time limit, and nothing more is started after one fails.  With
--parent-lib (the library of the parent commit, built elsewhere) a child that times that library's full decode and uniform
windows alternates with the children of this build, as tools/gpu/ab_multi.sh alternates settings on one box."""
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
    bsig = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p] + [ctypes.c_size_t] * 3 + [ctypes.c_void_p]
    if not args.no_boxes:
        lib.ebcc_hip_decode_frames_boxes.argtypes = bsig
        lib.ebcc_hip_decode_host_frames_boxes.argtypes = bsig
        lib.ebcc_hip_boxes_plan.argtypes = [ctypes.c_size_t] * 3 + [ctypes.c_void_p] + [ctypes.c_size_t] * 3 + [ctypes.c_void_p, ctypes.c_size_t]
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

    def ok(rc):
        assert rc == 0, lib.ebcc_hip_last_error()

    def window_calls(wins, streams=outs, lens=sizes, count=n):
        """one uniform-window call per window of the list, outputs one behind the other: (resident, host, floats put out)"""
        pix = [H * W if w is None else w[2] * w[3] for w in wins]

        def resident():
            at = 0
            for w, p in zip(wins, pix):
                d = d_out.data_ptr() + 4 * at
                ok(lib.ebcc_hip_decode_frames(ctx, streams, lens, count, d) if w is None else lib.ebcc_hip_decode_frames_window(ctx, streams, lens, count, *w, d))
                at += count * p

        def host(h_out):
            at = 0
            for w, p in zip(wins, pix):
                d = h_out.ctypes.data + 4 * at
                ok(lib.ebcc_hip_decode_host_frames(ctx, streams, lens, count, d) if w is None else
                   lib.ebcc_hip_decode_host_frames_window(ctx, streams, lens, count, *w, d))
                at += count * p
        return resident, host, count * sum(pix)

    def box_call(boxes, rows, cols):
        table = np.ascontiguousarray(np.asarray(boxes, np.uint64).reshape(-1, 3))

        def resident():
            ok(lib.ebcc_hip_decode_frames_boxes(ctx, outs, sizes, n, table.ctypes.data, len(table), rows, cols, d_out.data_ptr()))

        def host(h_out):
            ok(lib.ebcc_hip_decode_host_frames_boxes(ctx, outs, sizes, n, table.ctypes.data, len(table), rows, cols, h_out.ctypes.data))
        return resident, host, len(table) * rows * cols

    cases = [(name, window_calls([win]), win, None) for name, win in (CASES if not args.full_only else CASES[:1])]
    if not args.no_boxes:
        rng = np.random.default_rng(64)
        pts = [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(64)]
        track = [(f, 250 + (100 * f) // max(1, n - 1), ((W - 256) * f) // max(1, n - 1)) for f in range(n)]
        some = list(range(0, n, 8))
        s_outs, s_sizes = (ctypes.c_void_p * len(some))(*[outs[f] for f in some]), (ctypes.c_size_t * len(some))(*[sizes[f] for f in some])
        centre = CASES[2][1]
        cases += [("stations: 64 windows", window_calls([(r, c, 1, 1) for r, c in pts]), "64 calls", None),
                  ("stations: box list", box_call([(f, r, c) for f in range(n) for r, c in pts], 1, 1), None, ([(f, r, c) for f in range(n) for r, c in pts], 1, 1)),
                  ("track: bounding window", window_calls([(250, 0, 228, W)]), (250, 0, 228, W), None),
                  ("track: box list", box_call(track, 128, 256), None, (track, 128, 256)),
                  ("sparse: 32 streams", window_calls([centre], s_outs, s_sizes, len(some)), centre, None),
                  ("sparse: box list", box_call([(f, centre[0], centre[1]) for f in some], 128, 256), None, ([(f, centre[0], centre[1]) for f in some], 128, 256))]
        for name, win in CASES[1:]:                                      # (one path or two: the uniform windows through the box kernels)
            as_boxes = [(f, win[0], win[1]) for f in range(n)]
            cases.append((name + " as boxes", box_call(as_boxes, win[2], win[3]), None, (as_boxes, win[2], win[3])))
    for name, (resident, host_into, floats), win, listed in cases:

        def host():
            h_out = np.empty(floats, np.float32)                       # (a fresh pageable array every call, as a reader has)
            t0 = time.perf_counter()
            host_into(h_out)
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
            if listed is not None:
                boxes, rows, cols = listed
                table = np.ascontiguousarray(np.asarray(boxes, np.uint64).reshape(-1, 3))
                keep = np.zeros((n, 298), np.uint8)
                nb = lib.ebcc_hip_boxes_plan(H, W, n, table.ctypes.data, len(table), rows, cols, keep.ctypes.data, 298)
                assert nb == 298
                named = int(keep.any(axis=1).sum())
                # (code-blocks per named frame.  Rounds and launches are DERIVED from the code, not counted in the run: one decode
                #  slice - the default - of a context with n slots, the five fused levels of a 721 x 1440 frame per round, and the
                #  residual pass of at most 65535 records a launch)
                r["blocks_kept"], r["blocks"], r["frames_named"] = round(float(keep.sum()) / named, 1), nb, named
                r["rounds"] = -(-len(table) // n)
                r["launches"] = 5 * r["rounds"] + -(-len(table) // 65535)
            elif isinstance(win, str):
                r["blocks_kept"], r["blocks"] = win, 298
            elif win is None:
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
    ap.add_argument("--no-boxes", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    def med(v):
        return sorted(v)[len(v) // 2]

    for rnd in range(args.rounds):
        if args.parent_lib:
            pr = run_child(["--lib", os.path.abspath(args.parent_lib), "--no-boxes"], args.frames, args.reps)
            for name, _ in CASES:
                p = pr[name]
                print(f"round {rnd} [parent]     {name:24s}: resident {med(p['resident_ms']):8.2f} ms (min {min(p['resident_ms']):.2f}), t1_decode {p['t1_decode_ms']:6.2f} ms, "
                      f"host array {med(p['host_ms']):8.2f} ms (min {min(p['host_ms']):.2f})", flush=True)
        res = run_child([], args.frames, args.reps)
        full_bytes = res["full"].get("segment_bytes", 0)
        for name in [k for k in res if isinstance(res[k], dict)]:
            r = res[name]
            share = f"{100.0 * r['segment_bytes'] / full_bytes:5.1f} %" if full_bytes else "    ?"
            more = f"; frames named {r['frames_named']}, rounds {r['rounds']}, launches {r['launches']} (derived)" if "rounds" in r else ""
            print(f"round {rnd} [this build] {name:24s}: resident {med(r['resident_ms']):8.2f} ms (min {min(r['resident_ms']):.2f}), t1_decode {r['t1_decode_ms']:6.2f} ms in "
                  f"{r['t1_decode_spans']} spans, host array {med(r['host_ms']):8.2f} ms (min {min(r['host_ms']):.2f}); code-blocks kept {r['blocks_kept']}/{r['blocks']}, "
                  f"segment bytes {r.get('segment_bytes', 0)} ({share}){more}", flush=True)


if __name__ == "__main__":
    main()
