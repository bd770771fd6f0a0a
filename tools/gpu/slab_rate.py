"""GPU box: what a slab of a chunk container costs next to the only route without slab decode.  32 steps of
1801x3600 from the bench's field generator, coded by ebcc_encode_chunking_compat (base_cr 30, MAX_ERROR 0.5) with chunk dims (1, 1024,
1024) - its own default would leave the 1801 rows uncut - into 256 chunks, are read as (a) 32 x 400x600 across a four-chunk corner, (b) 32 x 128x256 inside one chunk, (c) the whole array -
through ebcc_decode_chunking_slab, and through ebcc_decode_chunking plus the crop with the library of the parent commit:
ms per call (median and minimum of --reps calls), and for the slabs the code-blocks and the segment bytes the tier-1 decoder
was given.

    python tools/gpu/slab_rate.py --parent-lib PATH [--rounds 2] [--reps 5] [--steps 32]

The container is made once by a child of this build and kept in a temporary file; every measurement is a child process under
its own time limit, the two libraries alternate, and nothing more is started after a child fails."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, W = 1801, 3600
CHILD_LIMIT = 400
SLABS = {"a 400x600 over 4 chunks": (824, 724, 400, 600), "b 128x256 in 1 chunk": (300, 400, 128, 256), "c whole array": (0, 0, H, W)}


class Slab(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in ("t0", "row0", "col0", "nt", "rows", "cols")]


def library(path):
    sys.path.insert(0, ROOT)
    from tests import _lib as L
    if path:
        L.PRODUCT_SO = path
    return L, L.product()


def make(args):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    import torch
    L, lib = library(None)
    import bench
    bench.H, bench.W = H, W                                              # (the generator takes the frame size from its module)
    frames = bench.synth_frames(torch, args.steps, torch.device("cuda", 0), seed=0).cpu().numpy()
    torch.cuda.synchronize()
    cfg = L.make_config((args.steps, H, W), (1, 1024, 1024), base_cr=bench.BASE_CR, error=bench.MAX_ERR, residual_type=L.MAX_ERROR)
    out = ctypes.c_void_p()
    n = lib.ebcc_encode_chunking_compat(frames.ctypes.data, ctypes.byref(cfg), ctypes.byref(out))
    assert n > 0, "ebcc_encode_chunking_compat failed"
    with open(args.make, "wb") as f:
        f.write(ctypes.string_at(out.value, n))
    lib.free_buffer(out)
    chunks = -(-H // 1024) * -(-W // 1024) * args.steps
    print(f"SLAB_RATE {json.dumps({'container_bytes': n, 'chunks': chunks})}", flush=True)


def child(args):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    import numpy as np
    L, lib = library(args.lib)
    buf = open(args.container, "rb").read()
    data = ctypes.create_string_buffer(buf, len(buf))
    nt = args.steps
    res = {}

    def whole():
        out = ctypes.c_void_p()
        n = lib.ebcc_decode_chunking(data, len(buf), ctypes.byref(out))
        assert n == nt * H * W
        return out

    def by_crop(slab):
        r0, c0, rows, cols = slab
        t0 = time.perf_counter()
        out = whole()
        a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_float)), (nt, H, W))
        got = a if (rows, cols) == (H, W) else np.ascontiguousarray(a[:, r0:r0 + rows, c0:c0 + cols])
        dt = time.perf_counter() - t0
        digest = int(got.view(np.uint32).sum(dtype=np.uint64))
        lib.free_buffer(out)
        return dt, digest

    def by_slab(slab):
        r0, c0, rows, cols = slab
        s = Slab(0, r0, c0, nt, rows, cols)
        out = ctypes.c_void_p()
        t0 = time.perf_counter()
        n = lib.ebcc_decode_chunking_slab(data, len(buf), ctypes.byref(s), ctypes.byref(out))
        dt = time.perf_counter() - t0
        assert n == nt * rows * cols, lib.ebcc_hip_last_error()
        a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_float)), (nt, rows, cols))
        digest = int(a.view(np.uint32).sum(dtype=np.uint64))
        lib.free_buffer(out)
        return dt, digest

    routes = [("crop", by_crop)]
    if not args.parent:
        lib.ebcc_decode_chunking_slab.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, L.c_void_pp]
        lib.ebcc_decode_chunking_slab.restype = ctypes.c_size_t
        routes.append(("slab", by_slab))
    for name, slab in SLABS.items():
        for route, fn in routes:
            if args.parent and route == "crop" and name[0] == "b":
                continue                                                   # (the parent's route costs the same for (a) and (b): the crop is a copy of a few MB)
            if not args.parent and route == "crop" and name[0] != "c":
                continue                                                   # (this build's full decode is timed once, for (c))
            fn(slab)                                                       # (warm-up: the engines are made)
            runs = [fn(slab) for _ in range(args.reps)]
            r = res.setdefault(name, {})
            r[route + "_ms"] = [round(1e3 * t, 2) for t, _ in runs]
            r[route + "_digest"] = runs[0][1]
            if route == "slab" and name[0] != "c":
                os.environ["EBCC_HIP_T1_STATS"] = "1"                      # (the decoder reports what it was given, on stderr)
                print(f"SLAB_STATS_BEGIN {name}", file=sys.stderr, flush=True)
                fn(slab)
                print("SLAB_STATS_END", file=sys.stderr, flush=True)
                del os.environ["EBCC_HIP_T1_STATS"]
    print("SLAB_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SLAB_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    res = json.loads(line[0].split(" ", 1)[1])
    name = None
    for ln in r.stderr.splitlines():                                       # per case: the sums over the batches' "t1 decode" lines between the markers
        if ln.startswith("SLAB_STATS_BEGIN "):
            name = ln.split(" ", 1)[1]
            res[name].update(blocks=0, segment_bytes=0, blocks_kept=0)
        elif ln.startswith("SLAB_STATS_END"):
            name = None
        elif name:
            m = re.search(r"t1 decode: (\d+) code-blocks, (\d+) bytes, (\d+) of them launched", ln)
            if m:
                res[name]["blocks"] += int(m.group(1)); res[name]["segment_bytes"] += int(m.group(2)); res[name]["blocks_kept"] += int(m.group(3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--parent-lib", help="libh5z_ebcc.so of the parent commit: its ebcc_decode_chunking plus the crop is the route to beat")
    ap.add_argument("--make", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--container", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--parent", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.make:
        return make(args)
    if args.child:
        return child(args)

    def med(v):
        return sorted(v)[len(v) // 2]

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "slab_rate.ebck")
        made = run_child(["--make", path, "--steps", str(args.steps)])
        print(f"container: {args.steps} x {H} x {W} in {made['container_bytes']} bytes, {made['chunks']} chunks of 1024 x 1024", flush=True)
        common = ["--child", "--container", path, "--steps", str(args.steps), "--reps", str(args.reps)]
        for rnd in range(args.rounds):
            pr = run_child(common + ["--parent", "--lib", os.path.abspath(args.parent_lib)]) if args.parent_lib else {}
            for name, r in pr.items():
                print(f"round {rnd} [parent]     {name:26s}: decode_chunking + crop {med(r['crop_ms']):9.2f} ms (min {min(r['crop_ms']):.2f})", flush=True)
            res = run_child(common)
            for name, r in res.items():
                same = "" if name not in pr or "slab_digest" not in r else ("; same bits as the parent's crop" if r["slab_digest"] == pr[name]["crop_digest"] else "; DIFFERS from the parent's crop")
                kept = f"; code-blocks kept {r['blocks_kept']}/{r['blocks']} of the chunks met, segment bytes {r['segment_bytes']}" if "blocks" in r else ""
                full = f"; this build's decode_chunking {med(r['crop_ms']):9.2f} ms (min {min(r['crop_ms']):.2f})" if "crop_ms" in r else ""
                print(f"round {rnd} [this build] {name:26s}: slab {med(r['slab_ms']):9.2f} ms (min {min(r['slab_ms']):.2f}){full}{kept}{same}", flush=True)


if __name__ == "__main__":
    main()
