"""GPU box: what the variables of one archive step cost as one call ("Frame groups").
8 groups x 32 frames of 721x1440 from the bench's field generator, every group its own tensor on the device; base_cr 30; the
groups' bounds: MAX_ERROR 0.5 / 0.25 / 1.0, RELATIVE_ERROR 1e-3 of the frame's range, RELATIVE_ERROR 1e-3 of the group's range,
NONE, and MAX_ERROR 0.5 and the group range once more.
  (a) the only route of the parent commit, with the parent's library: eight ebcc_hip_encode_frames calls, plus one
      ebcc_hip_array_range per group-range group (the caller restates the bound as MAX_ERROR with error * range);
  (b) this build: one ebcc_hip_encode_frames_groups call.
Both on a context of 256 frames.  ms per step, median and minimum of --reps steps, and whether the 256 streams are the same
bytes (total length and CRC over all of them in order).

    python tools/gpu/groups_rate.py --parent-lib PATH [--rounds 3] [--reps 5]

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
GROUPS, PER = 8, 32
REL_ERR = 1e-3
CHILD_LIMIT = 300
#        mode name, error, bound relative to the group's range
BOUNDS = [("MAX_ERROR", 0.5, 0), ("MAX_ERROR", 0.25, 0), ("MAX_ERROR", 1.0, 0), ("RELATIVE_ERROR", REL_ERR, 0), ("RELATIVE_ERROR", REL_ERR, 1),
          ("NONE", 0.0, 0), ("MAX_ERROR", 0.5, 0), ("RELATIVE_ERROR", REL_ERR, 1)]


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
    n = GROUPS * PER
    every = bench.synth_frames(torch, n, torch.device("cuda", 0), seed=0)
    tensors = [every[g * PER:(g + 1) * PER].clone().contiguous() for g in range(GROUPS)]          # (separate arrays, as a model's variables are)
    del every
    torch.cuda.synchronize()
    ctx = L.Context(n, H, W)
    lib.ebcc_hip_prepare.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert lib.ebcc_hip_prepare(ctx.ptr, n) == 0
    configs = [L.make_config((1, H, W), base_cr=bench.BASE_CR, error=err, residual_type=getattr(L, mode)) for mode, err, _ in BOUNDS]
    outs, sizes = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)()

    def digest():
        total, crc = 0, 0
        for i in range(n):
            crc = zlib.crc32(ctypes.string_at(outs[i], sizes[i]), crc)
            total += sizes[i]
            lib.free_buffer(outs[i])
        return total, crc

    def parent_route():
        lib.ebcc_hip_array_range.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        mm = np.zeros(2, np.float32)
        t0 = time.perf_counter()
        for g in range(GROUPS):
            cfg = configs[g]
            if BOUNDS[g][2]:
                assert lib.ebcc_hip_array_range(ctx.ptr, tensors[g].data_ptr(), PER * H * W, mm.ctypes.data) == 0
                cfg = L.make_config((1, H, W), base_cr=bench.BASE_CR, error=float(np.float32(BOUNDS[g][1]) * (mm[1] - mm[0])), residual_type=L.MAX_ERROR)
            o = (ctypes.c_void_p * PER).from_buffer(outs, g * PER * ctypes.sizeof(ctypes.c_void_p))
            s = (ctypes.c_size_t * PER).from_buffer(sizes, g * PER * ctypes.sizeof(ctypes.c_size_t))
            assert lib.ebcc_hip_encode_frames(ctx.ptr, tensors[g].data_ptr(), PER, ctypes.byref(cfg), o, s) == 0, lib.ebcc_hip_last_error()
        return time.perf_counter() - t0

    def groups_route():
        class Group(ctypes.Structure):                                   # ebcc_hip_frame_group, include/ebcc_hip.h
            _fields_ = [("frames", ctypes.c_void_p), ("n_frames", ctypes.c_size_t), ("config", L.CodecConfig), ("range_of_group", ctypes.c_int)]
        fn = lib.ebcc_hip_encode_frames_groups
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(Group), ctypes.c_size_t, L.c_void_pp, L.c_size_p]
        table = (Group * GROUPS)()
        for g in range(GROUPS):
            table[g].frames, table[g].n_frames, table[g].config, table[g].range_of_group = tensors[g].data_ptr(), PER, configs[g], BOUNDS[g][2]
        t0 = time.perf_counter()
        assert fn(ctx.ptr, table, GROUPS, outs, sizes) == 0, lib.ebcc_hip_last_error()
        return time.perf_counter() - t0

    route = parent_route if args.parent else groups_route
    route()                                                              # (warm-up)
    digest()
    ms, seen = [], set()
    for _ in range(args.reps):
        ms.append(round(1e3 * route(), 2))
        seen.add(digest())
    assert len(seen) == 1, "the streams differ from step to step"
    total, crc = seen.pop()
    ctx.close()
    print("GROUPS_RATE " + json.dumps({"ms": ms, "bytes": total, "crc": crc}), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("GROUPS_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    return json.loads(line[0].split(" ", 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: eight calls of its ebcc_hip_encode_frames are the route to beat")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--parent", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    def med(v):
        return sorted(v)[len(v) // 2]

    common = ["--reps", str(args.reps)]
    for rnd in range(args.rounds):
        a = run_child(common + ["--parent", "--lib", os.path.abspath(args.parent_lib)]) if args.parent_lib else None
        if a:
            print(f"round {rnd} (a) [parent]     eight calls + ranges: {med(a['ms']):8.2f} ms (min {min(a['ms']):.2f}), {a['bytes']} bytes", flush=True)
        b = run_child(common)
        same = "" if not a else ("; same bytes as (a)" if (a["bytes"], a["crc"]) == (b["bytes"], b["crc"]) else "; DIFFERS from (a)")
        print(f"round {rnd} (b) [this build] one groups call     : {med(b['ms']):8.2f} ms (min {min(b['ms']):.2f}), {b['bytes']} bytes{same}", flush=True)


if __name__ == "__main__":
    main()
