"""GPU box: what the spell decode costs on the bench workload ("Spell decode").
256 frames of 721x1440 from the bench's field generator, coded with base_cr 30 and MAX_ERROR 0.5 and resident as streams, a
context of 256 frames.
  y  ebcc_hip_reduce_shard, one bin, d_max and d_over - the parent's library (--parent-lib) and this build.  The yardstick: the
     same 256 frames decoded, every decoded sample read once.
  1  ebcc_hip_spell_shard, the runs alone (five arrays)
  2  ebcc_hip_spell_shard, the extremes alone (four arrays)
  3  ebcc_hip_spell_shard, all twelve arrays
  k  the kernels alone, timed with events (ebcc_hip_timing_read): "time_fold" of row y, "spell_fold" of rows 1 to 3, per call
ms are the median of --reps calls after one warm-up.  Every run asserts that d_max and d_events of row 3 are, byte for byte,
d_max and d_over of row y.

    python tools/gpu/spell_rate.py [--parent-lib PATH] [--rounds 2] [--reps 5]

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
ROWS = (("1", "runs", "the runs alone"), ("2", "extremes", "the extremes alone"), ("3", "all", "all twelve arrays"))


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
    frames = bench.synth_frames(torch, N, dev, seed=0)
    threshold = float(frames[0].float().mean())                             # (about half of the samples are events)
    torch.cuda.synchronize()
    outs, sizes = (ctypes.c_void_p * N)(), (ctypes.c_size_t * N)()
    assert lib.ebcc_hip_encode_shard(ctx.ptr, frames.data_ptr(), N, ctypes.byref(cfg), outs, sizes) == 0, lib.ebcc_hip_last_error()
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

    res = {"threshold": threshold}
    count = np.zeros(1, np.uint64)
    r_max, r_over = torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.int32, device=dev)
    st = B.TimeStats(1, H, W, None, None, None, r_max.data_ptr(), r_over.data_ptr(), threshold, count.ctypes.data)

    def reduce():
        return lib.ebcc_hip_reduce_shard(ctx.ptr, outs, sizes, N, None, 0, 0, ctypes.byref(st))

    res["reduce_ms"] = timed(reduce)
    res["reduce_kernel_ms"] = events(reduce, b"time_fold")
    if not args.parent:
        lib.ebcc_hip_spell_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(B.SpellStats)]
        lib.ebcc_hip_spell_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(B.SpellStats)]
        names = [n for family in B.SPELL_FAMILIES.values() for n in family]
        arrays = {n: torch.empty((H, W), dtype=torch.float32 if n in ("min", "max") else torch.int32, device=dev) for n in names}

        def stats(keep):
            s = B.SpellStats(1, H, W, threshold, 0, 6)
            s.count = count.ctypes.data
            for n in keep:
                setattr(s, "d_" + n, arrays[n].data_ptr())
            return s
        sets = {"runs": stats(B.SPELL_FAMILIES["runs"]), "extremes": stats(B.SPELL_FAMILIES["extremes"]), "all": stats(names)}
        for key, ps in sets.items():
            call = lambda: lib.ebcc_hip_spell_shard(ctx.ptr, outs, sizes, N, None, None, None, 0, 0, ctypes.byref(ps))  # noqa: E731
            res[f"spell_{key}_ms"] = timed(call)
            res[f"spell_{key}_kernel_ms"] = events(call, b"spell_fold")
        # the bytes: one call of each into accumulators set anew
        assert lib.ebcc_hip_time_stats_init(ctx.ptr, ctypes.byref(st)) == 0 and lib.ebcc_hip_spell_stats_init(ctx.ptr, ctypes.byref(sets["all"])) == 0
        assert reduce() == 0 and lib.ebcc_hip_spell_shard(ctx.ptr, outs, sizes, N, None, None, None, 0, 0, ctypes.byref(sets["all"])) == 0
        assert torch.equal(arrays["max"].view(torch.int32), r_max.view(torch.int32)) and torch.equal(arrays["events"], r_over), \
            "the spell decode and the reduce decode disagree"
        res["longest_max"] = int(arrays["longest"].max())
    for i in range(N):
        lib.free_buffer(outs[i])
    ctx.close()
    print("SPELL_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SPELL_RATE ")]
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
            print(f"round {rnd} [parent]     y reduce_shard, d_max + d_over: {med(a['reduce_ms']):8.2f} ms {a['reduce_ms']}; "
                  f"k time_fold {a['reduce_kernel_ms']:.3f} ms", flush=True)
        b = run_child(common)
        print(f"round {rnd} [this build] y reduce_shard, d_max + d_over: {med(b['reduce_ms']):8.2f} ms {b['reduce_ms']}; "
              f"k time_fold {b['reduce_kernel_ms']:.3f} ms", flush=True)
        y = a if a is not None else b
        for row, key, what in ROWS:
            print(f"round {rnd} [this build] {row} spell_shard, {what}: {med(b[f'spell_{key}_ms']):8.2f} ms {b[f'spell_{key}_ms']} "
                  f"= x {med(b[f'spell_{key}_ms']) / med(y['reduce_ms']):.3f} of {'the parent' if a is not None else 'this build'}'s row y; "
                  f"k spell_fold {b[f'spell_{key}_kernel_ms']:.3f} ms = x {b[f'spell_{key}_kernel_ms'] / b['reduce_kernel_ms']:.2f} of this build's time_fold",
                  flush=True)


if __name__ == "__main__":
    main()
