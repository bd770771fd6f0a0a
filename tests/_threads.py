"""The child process of tests/test_threads_gpu.py: `python -m tests._threads <scenario>` runs one scenario of concurrent callers.

Every scenario has the same shape.  The expected values are computed first, serially, on the CPU oracle (L.orc_encode,
L.orc_decode, and the numpy restatements the single-thread tests of a family use); then the threads start behind one
threading.Barrier, make a fixed, small number of calls each and keep what they got; after the joins the results are compared -
`==` on bytes, np.array_equal on fields.  Where the product's own serial result is at hand it is held against the oracle too,
first, so that a red run says which side moved.  One line is printed per finished phase:

    serial ok <seconds>     threads started     thread <k> done     joined <seconds>     compared

Nothing here waits with a time limit, sleeps or repeats itself: a deadlock in the library leaves the trail up to the last
line and is ended by the parent's time limit."""
import ctypes
import sys
import threading
import time
import traceback

import numpy as np

from tests import _fields as F
from tests import _hard_bound as HB
from tests import _lib as L
from tests.test_codec_gpu import api_decode, api_encode

T0 = time.perf_counter()


def say(*words):
    print(*words, flush=True)


def serial_ok():
    say("serial ok", f"{time.perf_counter() - T0:.2f}")


def run_threads(bodies):
    """bodies[k](barrier) on thread k, all released together by the barrier (a body may wait at it again: every body then
    does, the same number of times).  A body that raises breaks the barrier, so the others end instead of waiting for it."""
    barrier = threading.Barrier(len(bodies))
    failed = []

    def run(k):
        try:
            barrier.wait()
            bodies[k](barrier)
            say("thread", k, "done")
        except BaseException:                                        # noqa: B902
            failed.append(k)
            traceback.print_exc()
            barrier.abort()

    threads = [threading.Thread(target=run, args=(k,)) for k in range(len(bodies))]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    say("threads started")
    for t in threads:
        t.join()
    say("joined", f"{time.perf_counter() - t0:.2f}")
    assert not failed, f"threads {failed} raised"


def product_lib():
    lib = L.product()
    lib.ebcc_hip_release_engines.restype = None
    lib.ebcc_hip_prepare.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.ebcc_hip_prepare.restype = ctypes.c_int
    lib.ebcc_hip_device_count.restype = ctypes.c_int
    return lib


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


# ---- the reference API: a job is one array with its config ---------------------------------------------------------------------
class Job:
    """one ebcc_encode and one ebcc_decode: the array, its config, and what the oracle gives for them"""

    def __init__(self, data, mode, error, base_cr=20.0):
        self.data = np.ascontiguousarray(data, np.float32)
        shape = self.data.shape if self.data.ndim == 3 else (1,) + self.data.shape
        self.cfg = L.make_config(shape, base_cr=base_cr, error=error, residual_type=mode)
        self.want_stream = L.orc_encode(self.data, self.cfg)
        assert self.want_stream, "the oracle refused the input"
        self.want_field = L.orc_decode(self.want_stream)
        self.got_stream = self.got_field = None

    def run(self):
        self.got_stream = api_encode(self.data, self.cfg)
        self.got_field = api_decode(self.want_stream)

    def compare(self, what):
        # the product alone, after the threads have gone: if this differs the product or the oracle is wrong, threads or not
        assert api_encode(self.data, self.cfg) == self.want_stream, (what, "serial product stream differs from the oracle")
        assert np.array_equal(api_decode(self.want_stream), self.want_field), (what, "serial product field differs from the oracle")
        assert self.got_stream == self.want_stream, (what, "stream made beside other threads differs", len(self.got_stream), len(self.want_stream))
        assert np.array_equal(self.got_field, self.want_field), (what, "field decoded beside other threads differs")


def frame_jobs(k, h, w, n):
    """n jobs of thread k on h x w frames: thread 0 MAX_ERROR, 1 RELATIVE_ERROR, 2 NONE, 3 constant fields"""
    seeds = [10 * k + 100 * (h % 7) + i for i in range(n)]
    if k % 4 == 0:
        frames = [F.field("lowbit", h, w, seeds[0])] + [L.era5_like(h, w, s) for s in seeds[1:]]
        return [Job(x, L.MAX_ERROR, 0.05) for x in frames]
    if k % 4 == 1:
        frames = [L.era5_like(h, w, s, 1.2, 0.8) for s in seeds[:-1]] + [F.field("smooth", h, w, 2)]
        return [Job(x, L.RELATIVE_ERROR, 0.004) for x in frames[:n]]
    if k % 4 == 2:
        frames = [F.field("noise", h, w, seeds[0])] + [L.era5_like(h, w, s) for s in seeds[1:]]
        return [Job(x, L.NONE, 0.0, base_cr=10.0) for x in frames]
    return [Job(np.full((h, w), v, np.float32), L.MAX_ERROR, 0.1) for v in (7.0, 0.0, -3.25)[:n]]


def run_jobs(jobs):
    return lambda barrier: [j.run() for j in jobs]


def compare_jobs(per_thread):
    for k, jobs in enumerate(per_thread):
        for i, j in enumerate(jobs):
            j.compare(f"thread {k}, job {i}, shape {j.data.shape}")


def ref_one_geometry():
    """scenario 1: four threads, 64 x 96, one cached engine"""
    per_thread = [frame_jobs(k, 64, 96, 3) for k in range(4)]
    serial_ok()
    run_threads([run_jobs(jobs) for jobs in per_thread])
    compare_jobs(per_thread)


def ref_with_chunk():
    """scenario 1 again, thread 0 with one (4, 96, 160) chunk: the tiled path and chunk_engines beside one-frame calls"""
    chunk = np.stack([L.era5_like(96, 160, 40 + s, 1.1, 0.7) for s in range(4)])
    per_thread = [[Job(chunk, L.MAX_ERROR, 0.05)]] + [frame_jobs(k, 64, 96, 3) for k in range(1, 4)]
    serial_ok()
    run_threads([run_jobs(jobs) for jobs in per_thread])
    compare_jobs(per_thread)


GEOMETRIES = [(33, 47), (64, 96), (96, 160), (100, 130)]


def ref_four_geometries():
    """scenario 2: thread k begins on geometry k and moves to geometry k + 1: the engine map grows under contention"""
    per_thread = [[frame_jobs(k, *GEOMETRIES[(k + r) % 4], 1)[0] for r in range(2)] for k in range(4)]
    serial_ok()
    run_threads([run_jobs(jobs) for jobs in per_thread])
    compare_jobs(per_thread)


# ---- scenario 3: the Zarr codec on a thread pool -------------------------------------------------------------------------------
def zarr_pool():
    from concurrent.futures import ThreadPoolExecutor

    from ebcc_amd import EBCC_Filter
    from ebcc_amd.zarr_filter import EBCCZarrFilter
    kinds = [(64, 96, 12.0, "max_error_target", L.MAX_ERROR, 0.05), (96, 160, 20.0, "relative_error_target", L.RELATIVE_ERROR, 0.004)]
    codecs = [EBCCZarrFilter(EBCC_Filter(base_cr=cr, height=h, width=w, residual_opt=(name, err)).hdf_filter_opts) for h, w, cr, name, _m, err in kinds]
    chunks = []                                                       # (codec, data, oracle stream, oracle field), the geometries in turn
    for i in range(16):
        h, w, cr, _name, mode, err = kinds[i % 2]
        data = np.full((h, w), 4.5, np.float32) if i in (6, 7) else L.era5_like(h, w, 60 + i, 1.0 + 0.1 * (i % 4), 0.6 + 0.3 * (i % 3))
        want = L.orc_encode(data, L.make_config((1, h, w), base_cr=cr, error=err, residual_type=mode))
        assert want
        chunks.append((codecs[i % 2], data, want, L.orc_decode(want)))
    serial_ok()
    t0 = time.perf_counter()
    with ThreadPoolExecutor(4) as pool:
        say("threads started")
        streams = list(pool.map(lambda c: c[0].encode(c[1]), chunks))
        say("thread pool: 16 encodes done")
        flat = list(pool.map(lambda c: c[0].decode(c[2]), chunks))
        say("thread pool: 16 decodes done")
        outs = [np.full(c[1].shape, -1.0, np.float32) for c in chunks]
        back = list(pool.map(lambda a: a[0][0].decode(a[0][2], out=a[1]), zip(chunks, outs)))
        say("thread pool: 16 decodes into out= done")
    say("joined", f"{time.perf_counter() - t0:.2f}")
    for i, (codec, data, want, field) in enumerate(chunks):
        assert codec.encode(data) == want, (i, "serial product stream differs from the oracle")
        assert streams[i] == want, (i, "stream made on the pool differs")
        assert flat[i].shape == (data.size,) and np.array_equal(flat[i], field), (i, "field decoded on the pool differs")
        assert back[i] is outs[i] and np.array_equal(outs[i].ravel(), field), (i, "field decoded into out= on the pool differs")


# ---- scenario 4: one caller context per thread, a family of calls each --------------------------------------------------------
def context_families():
    from tests import _series as S
    from tests import test_audit_gpu as AG
    from tests import test_box_decode_gpu as BD
    from tests import test_hard_bound_gpu as HG
    from tests import test_reduce_gpu as RG
    from tests import test_series_gpu as SG
    from tests import test_window_gpu as T
    for m in (AG, BD, HG, RG, SG, T):
        m.lib()                                                       # (argument types declared once, before any thread calls)
    H, W = 64, 96
    x12 = np.array(HB.set_inputs("max_64x96")[:12])
    # family 0: encode_frames / decode_frames
    cfg0 = L.make_config((1, H, W), base_cr=20.0, error=0.02, residual_type=L.MAX_ERROR)
    want0 = [L.orc_encode(x, cfg0) for x in x12[:8]]
    field0 = np.stack([L.orc_decode(s).reshape(H, W) for s in want0])
    # family 1: a shard of twelve frames on a context of eight - the second engine set is made while the others run
    cfg1 = L.make_config((1, H, W), base_cr=20.0, error=0.004, residual_type=L.RELATIVE_ERROR)
    want1 = [L.orc_encode(x, cfg1) for x in x12]
    # family 2: the audit and the hard-bound encode, on the data of their own tests
    ax, astreams, adecoded, abound, awant = AG.mixed_batch()
    ax, astreams, adecoded, abound, awant = ax[:8], astreams[:8], adecoded[:8], abound[:8], awant[:8]
    hard_cfg = HG.set_config("max_64x96")
    _h, _w, _n, mode, err, cr, _env = HB.SETS["max_64x96"]
    loop = [HB.harden(x, mode, err, cr) for x in x12[:8]]
    assert [rep[3] for _s, rep, _hist in loop][:4] == [0, 1, 0, 2]           # (seeds 1 and 3 are coded again: the loop is taken)
    rc, audit_serial = AG.run_audit("shard", 8, ax, astreams, abound)         # (the sums in double have no numpy twin to the bit:
    assert rc == 0, last_error()                                              #  the product's own serial record stands in)
    for name in ("max_abs", "at", "n_over", "x_min", "x_max"):
        assert audit_serial[name].tobytes() == awant[name].tobytes(), ("serial product audit differs from numpy on the oracle's decode", name)
    # family 3: window, boxes, reduce and series of the same eight streams (two error modes, none, a constant frame)
    win = (9, 50, 40, 30)
    boxes = BD.twelve_per_frame(H, W, 8)
    bins = [f % 3 for f in range(8)]
    want_reduce = RG.expected(adecoded, bins, 3)
    w_row, w_pix = SG.weights(H, W, "both")
    threshold = float(np.median(adecoded[1]))
    want_series = S.expected(adecoded, SG.REGIONS, w_row, w_pix, threshold)
    serial_ok()
    got = {}

    def family0(barrier):
        with L.Context(8, H, W) as ctx:
            got["streams0"] = ctx.encode_frames(x12[:8], cfg0)
            got["field0"] = ctx.decode_frames(want0)

    def family1(barrier):
        with L.Context(8, H, W) as ctx:
            got["streams1"] = ctx.encode_shard(x12, cfg1)

    def family2(barrier):
        got["audit"] = AG.run_audit("shard", 8, ax, astreams, abound)         # (a context of eight frames of its own)
        got["hard"] = HG.encode_hard(x12[:8], hard_cfg, 8)                    # (and another)

    def family3(barrier):
        with L.Context(8, H, W) as ctx:
            got["window"] = T.window(ctx, astreams, win)
            got["boxes"] = BD.boxes_of(ctx, astreams, boxes, 16, 20)
            st = RG.Stats(3, H, W, base=1).init(ctx)
            got["reduce rc"] = RG.reduce(ctx, astreams, bins, st)
            got["reduce"], got["reduce guards"] = st.get(), st.sentinels_intact()
            pix = SG.Guarded(w_pix, 1)
            rc3, out = SG.series(ctx, astreams, SG.REGIONS, w_row, pix, threshold)
            got["series"] = (rc3, out.get(), out.margins_intact() and pix.untouched())

    run_threads([family0, family1, family2, family3])
    assert got["streams0"] == want0, "encode_frames beside other contexts"
    assert np.array_equal(got["field0"], field0), "decode_frames beside other contexts"
    assert got["streams1"] == want1, "encode_shard (two engine sets) beside other contexts"
    rc, audit = got["audit"]
    assert rc == 0 and audit.tobytes() == audit_serial.tobytes(), "audit beside other contexts"
    rc, streams, report = got["hard"]
    assert rc == 0 and streams == [s for s, _r, _h in loop], "hard-bound streams beside other contexts"
    assert report.tobytes() == HG.want_report(loop).tobytes(), "hard-bound report beside other contexts"
    assert T.same_bits(got["window"], T.crop(adecoded, win)), "window decode beside other contexts"
    assert T.same_bits(got["boxes"], BD.crops(adecoded, boxes, 16, 20)), "box decode beside other contexts"
    assert got["reduce rc"] == 0 and got["reduce guards"] and got["reduce"] == want_reduce, "reduce beside other contexts"
    rc, records, intact = got["series"]
    assert rc == 0 and intact, "series beside other contexts"
    for name in S.FIELDS:
        assert records[name].tobytes() == want_series[name].tobytes(), ("series beside other contexts", name)


# ---- scenario 5: one context, two threads ---------------------------------------------------------------------------------------
def shared_context():
    H, W = 64, 96
    cfgs = [L.make_config((1, H, W), base_cr=20.0, error=0.02, residual_type=L.MAX_ERROR),
            L.make_config((1, H, W), base_cr=12.0, error=0.004, residual_type=L.RELATIVE_ERROR)]
    xs = [HB.inputs(H, W, range(8)), HB.inputs(H, W, range(20, 26))]
    want = [[L.orc_encode(x, cfgs[k]) for x in xs[k]] for k in range(2)]
    fields = [np.stack([L.orc_decode(s).reshape(H, W) for s in want[k]]) for k in range(2)]
    serial_ok()
    got = [{}, {}]
    with L.Context(8, H, W) as ctx:
        def body(k):
            def run(barrier):
                got[k]["streams"] = ctx.encode_frames(xs[k], cfgs[k])       # (its own device buffers: L.Context allocates per call)
                got[k]["fields"] = ctx.decode_frames(want[k])
            return run
        run_threads([body(0), body(1)])
        for k in range(2):
            assert ctx.encode_frames(xs[k], cfgs[k]) == want[k], (k, "serial product streams differ from the oracle")
    for k in range(2):
        assert got[k]["streams"] == want[k], (k, "streams made on the shared context differ")
        assert np.array_equal(got[k]["fields"], fields[k]), (k, "fields decoded on the shared context differ")


# ---- scenario 6: the entry points that take no device lock, beside a running call -----------------------------------------------
def unlocked_helpers():
    jobs = frame_jobs(0, 64, 96, 3)
    pattern = (np.arange(1 << 16, dtype=np.uint32) * np.uint32(2654435761)).view(np.float32)
    serial_ok()
    got = {}

    def helper(barrier):
        with L.Context(4, 33, 47) as ctx:                               # (another geometry: made and destroyed beside the encode)
            got["workspace"] = L.product().ebcc_hip_workspace_bytes(ctx.ptr)
        d = L.DeviceArray(pattern)
        got["back"] = d.get(np.uint32, pattern.shape)
        d.free()

    run_threads([run_jobs(jobs), helper])
    assert got["workspace"] > 0
    assert np.array_equal(got["back"], pattern.view(np.uint32)), "a buffer copied up and back beside an encode"
    compare_jobs([jobs])


# ---- scenario 7: ebcc_hip_release_engines beside ebcc_encode / ebcc_decode --------------------------------------------------------
def release_beside_calls():
    lib = product_lib()
    per_thread = [frame_jobs(k, 64, 96, 3) for k in range(2)]
    serial_ok()

    def worker(jobs):
        def run(barrier):
            for r, j in enumerate(jobs):                                  # two calls a round: six calls
                if r:
                    barrier.wait()
                j.run()
        return run

    def releaser(barrier):
        for r in range(3):                                                # once after each barrier the workers pass
            if r:
                barrier.wait()
            lib.ebcc_hip_release_engines()

    run_threads([worker(per_thread[0]), worker(per_thread[1]), releaser])
    compare_jobs(per_thread)


# ---- scenario 8: the last error is per thread -----------------------------------------------------------------------------------
def last_error_per_thread():
    lib = product_lib()
    job = frame_jobs(0, 64, 96, 1)[0]
    serial_ok()
    got = {}
    with L.Context(4, 64, 96) as ctx:
        def refused(barrier):
            got["rc"] = lib.ebcc_hip_prepare(ctx.ptr, ctx.max_frames + 1)     # refused on the host, before any device work
            barrier.wait()
            got["a"] = last_error()

        def succeeds(barrier):
            job.run()
            barrier.wait()
            got["b"] = last_error()

        run_threads([refused, succeeds])
    say("texts", repr(got["a"]), repr(got["b"]))
    assert got["rc"] == 1 and "ebcc_hip_prepare" in got["a"], got
    assert "ebcc_hip_prepare" not in got["b"], got
    job.compare("the thread that succeeds")


# ---- scenario 9: ebcc_hip_create and the caller's current device ------------------------------------------------------------------
def create_keeps_device():
    import torch
    lib = product_lib()
    assert lib.ebcc_hip_device_count() >= 2, "two devices are needed"
    serial_ok()
    torch.cuda.set_device(0)
    ctx = lib.ebcc_hip_create(1, 4, 64, 96)
    assert ctx, last_error()
    after_create = torch.cuda.current_device()
    lib.ebcc_hip_destroy(ctx)
    after_destroy = torch.cuda.current_device()
    say("device after create", after_create, "after destroy", after_destroy)
    assert after_create == 0 and after_destroy == 0


SCENARIOS = {f.__name__: f for f in (ref_one_geometry, ref_with_chunk, ref_four_geometries, zarr_pool, context_families, shared_context,
                                     unlocked_helpers, release_beside_calls, last_error_per_thread, create_keeps_device)}

if __name__ == "__main__":
    L.oracle().orc_set_j2k_backend(0)
    product_lib()
    SCENARIOS[sys.argv[1]]()
    say("compared")
