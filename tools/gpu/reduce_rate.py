"""GPU box: what the reduce decode costs on the bench workload ("Reduce decode").
256 frames of 721x1440 from the bench's field generator, coded with base_cr 30 and MAX_ERROR 0.5 and resident as streams, a
context of 256 frames.
  1  ebcc_hip_decode_shard into [256][H][W] on the device: the parent's library (--parent-lib) and this build - the yardstick
  2  ebcc_hip_reduce_shard, one bin, all five accumulators
  3  the same with bins = f % 24 (a daily cycle from hourly steps)
  4  the same with one bin and a 200 x 300 window
  5  the fold's launches alone (ebcc_hip_time_fold on the decoded frames, timed with events: ebcc_hip_timing_read "time_fold"),
     one bin and 24, with the bytes of the frames over the time; beside it the audit's statistics pass over the same frames
     (ebcc_hip_frame_errors, "frame_errors"), which reads them twice
ms are the median of --reps calls after one warm-up.  The reduce call's accumulators are compared, byte for byte, with the fold
of what ebcc_hip_decode_shard gave.

    python tools/gpu/reduce_rate.py [--parent-lib PATH] [--rounds 1] [--reps 5]

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
WINDOW = (260, 570, 200, 300)                          # row0, col0, rows, cols
FIELDS = (("d_sum", 8), ("d_sum_sq", 8), ("d_min", 4), ("d_max", 4), ("d_over", 4))


class TimeStats(ctypes.Structure):
    """ebcc_hip_time_stats, include/ebcc_hip.h"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("d_sum", ctypes.c_void_p), ("d_sum_sq", ctypes.c_void_p), ("d_min", ctypes.c_void_p), ("d_max", ctypes.c_void_p),
                ("d_over", ctypes.c_void_p), ("threshold", ctypes.c_float), ("count", ctypes.c_void_p)]


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
        lib.ebcc_hip_time_stats_init.argtypes = [ctypes.c_void_p, ctypes.POINTER(TimeStats)]
        lib.ebcc_hip_time_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(TimeStats)]
        lib.ebcc_hip_reduce_shard.argtypes = [ctypes.c_void_p, L.c_void_pp, L.c_size_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.POINTER(TimeStats)]
        lib.ebcc_hip_frame_errors.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_void_p]
        lib.ebcc_hip_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.ebcc_hip_timing_read.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]

        class Stats:
            def __init__(self, n_bins, rows, cols):
                self.count = np.zeros(n_bins, np.uint64)
                self.c = TimeStats(n_bins, rows, cols, None, None, None, None, None, 280.0, self.count.ctypes.data)
                self.bufs = {name: L.DeviceArray(nbytes=n_bins * rows * cols * size) for name, size in FIELDS}
                for name, b in self.bufs.items():
                    setattr(self.c, name, b.ptr)

            def init(self):
                assert lib.ebcc_hip_time_stats_init(ctx.ptr, ctypes.byref(self.c)) == 0, lib.ebcc_hip_last_error()
                return self

            def bytes(self):
                return [b.get(np.uint8, (b.nbytes,)).tobytes() for b in self.bufs.values()] + [self.count.tobytes()]

            def free(self):
                for b in self.bufs.values():
                    b.free()

        def events(name, call):
            lib.ebcc_hip_timing_enable(ctx.ptr, 1)
            for _ in range(args.reps):
                assert call() == 0
            total, launches = ctypes.c_double(), ctypes.c_long()
            lib.ebcc_hip_timing_read(ctx.ptr, name, ctypes.byref(total), ctypes.byref(launches))
            lib.ebcc_hip_timing_enable(ctx.ptr, 0)
            return total.value / max(1, launches.value)

        frame_bytes = N * H * W * 4
        for key, n_bins in (("one", 1), ("day", 24)):
            bins = (np.arange(N) % n_bins).astype(np.uint32)
            st = Stats(n_bins, H, W).init()
            assert lib.ebcc_hip_reduce_shard(ctx.ptr, outs, sizes, N, bins.ctypes.data, 0, 0, ctypes.byref(st.c)) == 0, lib.ebcc_hip_last_error()
            got = st.bytes()
            st.init()
            assert lib.ebcc_hip_time_fold(ctx.ptr, dec.data_ptr(), N, bins.ctypes.data, ctypes.byref(st.c)) == 0, lib.ebcc_hip_last_error()
            assert st.bytes() == got, "the reduce call and the fold of the decoded frames disagree"
            # (the timed calls add to what the accumulators hold: the work is the same)
            res[f"reduce_{key}_ms"] = timed(lambda: lib.ebcc_hip_reduce_shard(ctx.ptr, outs, sizes, N, bins.ctypes.data, 0, 0, ctypes.byref(st.c)))
            res[f"fold_{key}_call_ms"] = timed(lambda: lib.ebcc_hip_time_fold(ctx.ptr, dec.data_ptr(), N, bins.ctypes.data, ctypes.byref(st.c)))
            ms = events(b"time_fold", lambda: lib.ebcc_hip_time_fold(ctx.ptr, dec.data_ptr(), N, bins.ctypes.data, ctypes.byref(st.c)))
            res[f"fold_{key}_event_ms"] = ms
            res[f"fold_{key}_tb_s"] = frame_bytes / (ms * 1e-3) / 1e12
            st.free()
        row0, col0, rows, cols = WINDOW
        st = Stats(1, rows, cols).init()
        assert lib.ebcc_hip_reduce_shard(ctx.ptr, outs, sizes, N, None, row0, col0, ctypes.byref(st.c)) == 0, lib.ebcc_hip_last_error()
        got = st.bytes()
        crop = dec[:, row0:row0 + rows, col0:col0 + cols].contiguous()
        torch.cuda.synchronize()
        st.init()
        assert lib.ebcc_hip_time_fold(ctx.ptr, crop.data_ptr(), N, None, ctypes.byref(st.c)) == 0, lib.ebcc_hip_last_error()
        assert st.bytes() == got, "the window reduce and the fold of the crop disagree"
        res["reduce_window_ms"] = timed(lambda: lib.ebcc_hip_reduce_shard(ctx.ptr, outs, sizes, N, None, row0, col0, ctypes.byref(st.c)))
        st.free()
        report = np.zeros(N, [("max_abs", "<f4"), ("at", "<u4"), ("n_over", "<u8"), ("sum", "<f8"), ("sum_sq", "<f8"), ("x_min", "<f4"), ("x_max", "<f4")])
        ms = events(b"frame_errors", lambda: lib.ebcc_hip_frame_errors(ctx.ptr, frames.data_ptr(), dec.data_ptr(), N, H, W, None, report.ctypes.data))
        res["stats_event_ms"] = ms
        res["stats_tb_s"] = 2 * frame_bytes / (ms * 1e-3) / 1e12
    for i in range(N):
        lib.free_buffer(outs[i])
    ctx.close()
    print("REDUCE_RATE " + json.dumps(res), flush=True)


def run_child(extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("REDUCE_RATE ")]
    if r.returncode != 0 or len(line) != 1:
        print(f"child {' '.join(extra)} failed with status {r.returncode}; nothing more is started\n{r.stdout[-1500:]}{r.stderr[-3000:]}", flush=True)
        sys.exit(1)
    return json.loads(line[0].split(" ", 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1)
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
        if args.parent_lib:
            a = run_child(common + ["--parent", "--lib", os.path.abspath(args.parent_lib)])
            print(f"round {rnd} [parent]     decode_shard {med(a['decode_ms']):8.2f} ms", flush=True)
        b = run_child(common)
        print(f"round {rnd} [this build] decode_shard {med(b['decode_ms']):8.2f} ms; reduce_shard: one bin {med(b['reduce_one_ms']):.2f} ms, "
              f"bins f % 24 {med(b['reduce_day_ms']):.2f} ms, one bin of a {WINDOW[2]} x {WINDOW[3]} window {med(b['reduce_window_ms']):.2f} ms; "
              f"time_fold call: one bin {med(b['fold_one_call_ms']):.2f} ms, 24 bins {med(b['fold_day_call_ms']):.2f} ms; its launches alone: one bin "
              f"{b['fold_one_event_ms']:.3f} ms = {b['fold_one_tb_s']:.2f} TB/s of frames, 24 bins {b['fold_day_event_ms']:.3f} ms = {b['fold_day_tb_s']:.2f} TB/s; "
              f"frame_errors launches {b['stats_event_ms']:.3f} ms = {b['stats_tb_s']:.2f} TB/s over two reads", flush=True)


if __name__ == "__main__":
    main()
