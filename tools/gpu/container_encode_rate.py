"""GPU box: what a container of an array that lies on the device costs ("Container encode from the device").
32 steps of 1801x3600 from the bench's field generator stay on the device; chunks (1, 1024, 1024), 256 of them; base_cr 30.
  (a) the only route of the parent commit: ebcc_hip_download of the array, then ebcc_encode_chunking on the host copy - with the
      parent's library;
  (b) ebcc_hip_encode_container on the array where it lies.
Both under MAX_ERROR 0.5 through the plain forms and under RELATIVE_ERROR 0.005 through the compat forms (the global range: a
single-threaded host scan in (a), a kernel in (b)).  ms per call, median and minimum of --reps calls, and whether the containers
are the same bytes.  For this build also the gather launches alone - all 256 chunks, timed with events on the context's stream -
set against the bytes they read and write.

    python tools/gpu/container_encode_rate.py --parent-lib PATH [--rounds 2] [--reps 5] [--steps 32]

Every measurement is a child process under its own time limit, the two libraries alternate, and nothing more is started after a
child fails."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, W, CH, CW = 1801, 3600, 1024, 1024
REL_ERR = 0.005
CHILD_LIMIT = 400


def child(args):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from tests import _lib as L
    if args.lib:
        L.PRODUCT_SO = args.lib
    lib = L.product()
    import bench
    bench.H, bench.W = H, W                                              # (the generator takes the frame size from its module)
    nt = args.steps
    frames = bench.synth_frames(torch, nt, torch.device("cuda", 0), seed=0).contiguous()
    torch.cuda.synchronize()
    assert frames.dtype == torch.float32 and tuple(frames.shape) == (nt, H, W)
    chunks = nt * -(-H // CH) * -(-W // CW)
    lib.ebcc_hip_download.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    ctx = L.Context(1 if args.parent else chunks, CH, CW)                # (a): for the download alone; the encode keeps its own engines
    configs = {"MAX_ERROR 0.5, plain": (L.make_config((nt, H, W), (1, CH, CW), base_cr=bench.BASE_CR, error=bench.MAX_ERR, residual_type=L.MAX_ERROR), 0),
               f"RELATIVE_ERROR {REL_ERR}, compat": (L.make_config((nt, H, W), (1, CH, CW), base_cr=bench.BASE_CR, error=REL_ERR, residual_type=L.RELATIVE_ERROR), 1)}

    def parent_route(cfg, compat):
        t0 = time.perf_counter()
        host = np.empty((nt, H, W), np.float32)
        assert lib.ebcc_hip_download(ctx.ptr, host.ctypes.data, frames.data_ptr(), host.nbytes) == 0
        out = ctypes.c_void_p()
        n = (lib.ebcc_encode_chunking_compat if compat else lib.ebcc_encode_chunking)(host.ctypes.data, ctypes.byref(cfg), ctypes.byref(out))
        dt = time.perf_counter() - t0
        assert n > 0
        crc = zlib.crc32(ctypes.string_at(out.value, n))
        lib.free_buffer(out)
        return dt, n, crc

    def resident_route(cfg, compat):
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        t0 = time.perf_counter()
        rc = lib.ebcc_hip_encode_container(ctx.ptr, frames.data_ptr(), ctypes.byref(cfg), compat, ctypes.byref(out), ctypes.byref(n))
        dt = time.perf_counter() - t0
        assert rc == 0, lib.ebcc_hip_last_error()
        crc = zlib.crc32(ctypes.string_at(out.value, n.value))
        lib.free_buffer(out)
        return dt, n.value, crc

    res = {}
    if not args.parent:
        lib.ebcc_hip_encode_container.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(L.CodecConfig), ctypes.c_int, L.c_void_pp, L.c_size_p]
        lib.ebcc_hip_gather_chunks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, L.c_size_p, L.c_size_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
        lib.ebcc_hip_array_range.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.ebcc_hip_stream.restype = ctypes.c_void_p
        lib.ebcc_hip_stream.argtypes = [ctypes.c_void_p]
        stream = torch.cuda.ExternalStream(lib.ebcc_hip_stream(ctx.ptr))
        staged = torch.empty(chunks * CH * CW, dtype=torch.float32, device="cuda")
        dims, cd = (ctypes.c_size_t * 3)(nt, H, W), (ctypes.c_size_t * 3)(1, CH, CW)
        mm = np.zeros(2, np.float32)

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert call() == 0, lib.ebcc_hip_last_error()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        gather = lambda: lib.ebcc_hip_gather_chunks(ctx.ptr, frames.data_ptr(), dims, cd, 0, chunks, staged.data_ptr())   # noqa: E731
        scan = lambda: lib.ebcc_hip_array_range(ctx.ptr, frames.data_ptr(), nt * H * W, mm.ctypes.data)                  # noqa: E731
        for name, call, moved in (("gather", gather, 4 * (nt * H * W + chunks * CH * CW)), ("range", scan, 4 * nt * H * W)):
            timed(call)
            res[name] = {"ms": [round(timed(call), 4) for _ in range(args.reps)], "bytes": moved}
    route = parent_route if args.parent else resident_route
    for name, (cfg, compat) in configs.items():
        route(cfg, compat)                                               # (warm-up: the engines are made)
        runs = [route(cfg, compat) for _ in range(args.reps)]
        res[name] = {"ms": [round(1e3 * r[0], 2) for r in runs], "bytes": runs[0][1], "crc": runs[0][2]}
    ctx.close()
    print("CONTAINER_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CONTAINER_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    return json.loads(line[0].split(" ", 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: ebcc_hip_download plus its ebcc_encode_chunking is the route to beat")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--parent", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    def med(v):
        return sorted(v)[len(v) // 2]

    common = ["--steps", str(args.steps), "--reps", str(args.reps)]
    for rnd in range(args.rounds):
        pr = run_child(common + ["--parent", "--lib", os.path.abspath(args.parent_lib)]) if args.parent_lib else {}
        for name, r in pr.items():
            print(f"round {rnd} [parent]     {name:32s}: download + host encode {med(r['ms']):9.2f} ms (min {min(r['ms']):.2f}), {r['bytes']} bytes", flush=True)
        res = run_child(common)
        for name, r in res.items():
            if name in ("gather", "range"):
                print(f"round {rnd} [this build] {name:32s}: {med(r['ms']):9.4f} ms (min {min(r['ms']):.4f}) for {r['bytes']} bytes read and written: "
                      f"{r['bytes'] / med(r['ms']) / 1e6:.0f} GB/s", flush=True)
                continue
            same = "" if name not in pr else ("; same bytes as the parent's" if (r["bytes"], r["crc"]) == (pr[name]["bytes"], pr[name]["crc"]) else "; DIFFERS from the parent's")
            print(f"round {rnd} [this build] {name:32s}: encode_container       {med(r['ms']):9.2f} ms (min {min(r['ms']):.2f}), {r['bytes']} bytes{same}", flush=True)


if __name__ == "__main__":
    main()
