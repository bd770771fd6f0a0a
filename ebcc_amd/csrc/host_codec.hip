// host_codec.hip - the reference's C API (include/ebcc_codec.h) on top of the MI355X engine: engines per device and
// frame geometry, concurrent slices and alternating engine sets of a batch, host <-> device copies, the EBCK chunk
// container (/root/reference/src/ebcc_codec.c:920-1090, :1322-1449), and the batch entry points of include/ebcc_hip.h.
// Its kernels are in array_stats.hip: the chunk gather, the range of an array (and of many) on the device, the per-frame error
// statistics of the audit and the hard-bound encode, the fold over time of the reduce decode, the area series.
// The frame codec itself is batch_codec.hip, the HDF5 plugin h5z_filter.hip, the host services host_pool.hip (host.hpp).
// There is no CPU fallback: without a HIP device every entry point fails loudly.
#include <climits>
#include "array_stats.hpp"
#include "regrid.hpp"
#include "quantile.hpp"
#include "time_map.hpp"
#include "pair_stats.hpp"
#include "spell_stats.hpp"
#include "time_walk.hpp"

using namespace ebcc;

namespace {

// ================================================================================================
// devices and the context cache: one engine per (device, frame geometry), grown on demand
// ================================================================================================
// The reference-compatible entry points have no device argument.  They run on
//   EBCC_HIP_DEVICE=<n>          if set, else on the calling thread's current HIP device (what torch.cuda.set_device or
//                                hipSetDevice chose; 0 in a process that never chose), and
//   EBCC_HIP_DEVICES=all|a,b,..  lets the chunking entry points spread their chunk list over several devices (default:
//                                all visible devices in a stand-alone process, the one device above when the process is
//                                one rank of a multi-process job - LOCAL_WORLD_SIZE / WORLD_SIZE > 1).
// Every entry point makes its device current for the call and restores the caller's on return.
int resolve_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return 0;         // (create_engine reports the missing device)
    if (const char *e = getenv("EBCC_HIP_DEVICE")) { int d = atoi(e); return d >= 0 && d < n ? d : 0; }
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) d = 0;
    return d;
}
bool multi_process_job()
{
    for (const char *v : {"LOCAL_WORLD_SIZE", "WORLD_SIZE"})
        if (const char *e = getenv(v)) if (atoi(e) > 1) return true;
    return false;
}
std::vector<int> device_list()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return {0};
    const char *e = getenv("EBCC_HIP_DEVICES");
    std::vector<int> out;
    if (e && strcmp(e, "all") != 0) {
        for (const char *p = e; *p;) {
            char *end;
            long d = strtol(p, &end, 10);
            if (end == p) break;
            // (a device named twice counts once - unless EBCC_HIP_DEVICES_KEEP_REPEATS=1, the tests' way to drive the
            //  several-devices path of run_on_devices on a one-GPU box: the per-device lock then serialises the blocks)
            static const bool keep = getenv("EBCC_HIP_DEVICES_KEEP_REPEATS") != nullptr;
            if (d >= 0 && d < n && (keep || std::find(out.begin(), out.end(), (int) d) == out.end())) out.push_back((int) d);
            p = *end == ',' ? end + 1 : end;
        }
    } else if (e || !multi_process_job()) {
        for (int d = 0; d < n; d++) out.push_back(d);
    }
    if (out.empty()) out.push_back(resolve_device());
    return out;
}
struct DeviceScope {               // the engine's device for the duration of a call, the caller's afterwards
    int prev = -1;
    explicit DeviceScope(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; EBCC_HIP_CHECK(hipSetDevice(dev)); }
    ~DeviceScope() { if (prev >= 0) hipSetDevice(prev); }
};
// One lock per device (HDF5 serialises filter calls anyway; a multi-threaded writer gets one call per device at a time).
std::mutex &device_mutex(int dev)
{
    static std::mutex m[64];
    return m[dev & 63];
}

// The prologue of every entry point that works on a device: the device's lock, the device current (DeviceScope), and an
// exception turned into a logged failure that returns `fail`.  on_codec also needs libzstd, as every encode and the decode
// of a residual layer do.
template <class R, class Fn>
R on_device(int device, R fail, Fn &&fn)
{
    try {
        std::lock_guard<std::mutex> lock(device_mutex(device));
        DeviceScope scope(device);
        return fn();
    } catch (const std::exception &e) {
        log_fatal("MI355X engine failure: %s", e.what());
        set_error("%s", e.what());
        return fail;
    }
}
template <class R, class Fn>
R on_codec(int device, R fail, Fn &&fn)
{
    return on_device(device, fail, [&]() -> R {
        if (!zstd().ok) { log_fatal("libzstd not available"); return fail; }
        return fn();
    });
}

std::mutex g_map_mutex;
std::map<std::tuple<int, int, int, int>, ebcc_hip_ctx *> g_ctx;

// `period` > 1: the frames are the tiles of images of that many tiles each, every tile position with its own
// JPEG 2000 geometry (j2k.hpp).  Called with the device's lock held and the device current.
ebcc_hip_ctx *get_context(int device, int H, int W, size_t frames, int period = 1)
{
    std::lock_guard<std::mutex> lock(g_map_mutex);
    auto key = std::make_tuple(device, H, W, period);
    auto it = g_ctx.find(key);
    if (it != g_ctx.end() && it->second->max_frames >= frames) return it->second;
    if (it != g_ctx.end()) { ebcc_hip_destroy(it->second); g_ctx.erase(it); }
    ebcc_hip_ctx *c = create_engine(device, frames, (size_t) H, (size_t) W, period);
    if (!c) {                                                   // out of device memory: drop this device's engines of other geometries
        bool dropped = false;
        for (auto i = g_ctx.begin(); i != g_ctx.end();)
            if (std::get<0>(i->first) == device) { ebcc_hip_destroy(i->second); i = g_ctx.erase(i); dropped = true; } else ++i;
        if (dropped) c = create_engine(device, frames, (size_t) H, (size_t) W, period);
    }
    if (c) g_ctx[key] = c;
    return c;
}

// the device image of a host array handed to the reference API: kept in the context between calls
float *io_buffer(ebcc_hip_ctx *ctx, size_t bytes) { return (float *) ctx->io.reserve(bytes, false, true); }

// A pageable host array <-> the device image, through two pinned buffers: the DMA engine fills (or drains) one while a few
// host threads copy the other to (or from) the caller's memory.  hipMemcpy on pageable memory stages through one internal
// buffer on one thread: ~10 GB/s, 100 ms for the 1.06 GB of a 256-frame batch - four times the decode itself.
constexpr size_t kBounceBytes = (size_t) 32 << 20;
static void host_copy_parallel(void *dst, const void *src, size_t bytes)
{
    const size_t nthreads = std::min<size_t>(8, std::max<size_t>(1, bytes >> 20));
    std::vector<std::thread> pool;
    size_t started = 1;
    try {
        for (size_t t = 1; t < nthreads; t++, started++)
            pool.emplace_back([=]() { const size_t lo = bytes / nthreads * t, hi = t + 1 == nthreads ? bytes : bytes / nthreads * (t + 1);
                                      memcpy((char *) dst + lo, (const char *) src + lo, hi - lo); });
    } catch (const std::exception &) {}                                 // (thread limit: this thread copies what is left)
    memcpy(dst, src, bytes / nthreads);
    if (started < nthreads) { const size_t lo = bytes / nthreads * started; memcpy((char *) dst + lo, (const char *) src + lo, bytes - lo); }
    for (auto &t : pool) t.join();
}
static void copy_pageable(ebcc_hip_ctx *ctx, void *host, void *dev, size_t bytes, bool to_host)
{
    if (bytes < 2 * kBounceBytes) {
        EBCC_HIP_CHECK(hipMemcpy(to_host ? host : dev, to_host ? dev : host, bytes, to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice));
        return;
    }
    if (!ctx->h_bounce) EBCC_HIP_CHECK(hipHostMalloc((void **) &ctx->h_bounce, 2 * kBounceBytes));
    hipStream_t s = ctx->stream;
    const size_t chunks = (bytes + kBounceBytes - 1) / kBounceBytes;
    auto len = [&](size_t i) { return std::min(kBounceBytes, bytes - i * kBounceBytes); };
    if (to_host) {
        EBCC_HIP_CHECK(hipMemcpyAsync(ctx->h_bounce, dev, len(0), hipMemcpyDeviceToHost, s));
        for (size_t i = 0; i < chunks; i++) {
            wait_stream(s);                                       // chunk i has arrived
            if (i + 1 < chunks)
                EBCC_HIP_CHECK(hipMemcpyAsync(ctx->h_bounce + ((i + 1) & 1) * kBounceBytes, (char *) dev + (i + 1) * kBounceBytes, len(i + 1), hipMemcpyDeviceToHost, s));
            host_copy_parallel((char *) host + i * kBounceBytes, ctx->h_bounce + (i & 1) * kBounceBytes, len(i));
        }
    } else {
        for (size_t i = 0; i < chunks; i++) {
            host_copy_parallel(ctx->h_bounce + (i & 1) * kBounceBytes, (const char *) host + i * kBounceBytes, len(i));
            if (i >= 1) wait_stream(s);                           // (chunk i - 1 has left: its buffer is filled next)
            EBCC_HIP_CHECK(hipMemcpyAsync((char *) dev + i * kBounceBytes, ctx->h_bounce + (i & 1) * kBounceBytes, len(i), hipMemcpyHostToDevice, s));
        }
        wait_stream(s);
    }
}

// A fresh allocation of hundreds of MB is unmapped pages: a download into it would fault them in one by one on the copying
// threads.  Huge pages where the system grants them (512 x fewer faults), and a few host threads that touch the pages
// meanwhile (while the GPU decodes).
constexpr size_t kFreshPagesBytes = (size_t) 64 << 20;
void huge_pages(void *p, size_t bytes)
{
    if (bytes < kFreshPagesBytes) return;
    const uintptr_t a = ((uintptr_t) p + ((size_t) 2 << 20) - 1) & ~(((uintptr_t) 2 << 20) - 1), e = ((uintptr_t) p + bytes) & ~(((uintptr_t) 2 << 20) - 1);
    if (e > a) madvise((void *) a, e - a, MADV_HUGEPAGE);
}
struct Prefault {
    std::vector<std::thread> pool;
    Prefault(void *p, size_t bytes)
    {
        const size_t nthreads = bytes >= kFreshPagesBytes ? std::min<size_t>(16, std::max(1u, (unsigned) entropy_threads(1))) : 0;
        huge_pages(p, bytes);
        try {
            for (size_t t = 0; t < nthreads; t++)
                pool.emplace_back([=]() {
                    volatile char *c = (volatile char *) p;
                    const size_t lo = bytes / nthreads * t, hi = t + 1 == nthreads ? bytes : bytes / nthreads * (t + 1);
                    for (size_t i = lo; i < hi; i += 4096) c[i] = 0;
                });
        } catch (const std::exception &) {}                         // (no thread to be had: the download faults the pages in itself)
    }
    std::mutex m;                                                   // (one device thread per device may come here)
    void join() { std::lock_guard<std::mutex> g(m); for (auto &t : pool) if (t.joinable()) t.join(); }
    ~Prefault() { join(); }
};

// Frames per device batch of the host-pointer entry points: EBCC_HIP_MAX_BATCH (default 256), reduced for large
// frames so that an engine's workspace (about 160 bytes per pixel and frame with the worst-case slots) stays
// under ~48 GB, and never more than a context holds (kMaxEngineFrames frames: chunks of `tiles` frames count as that many).
size_t batch_capacity(size_t n_pix, size_t tiles = 1)
{
    const char *e = getenv("EBCC_HIP_MAX_BATCH");
    size_t v = e ? strtoul(e, nullptr, 10) : 256;
    if (!v) v = 256;
    const size_t fit = ((size_t) 48 << 30) / (n_pix * 160 + 1);
    return std::max<size_t>(1, std::min({v, fit, ebcc::kMaxEngineFrames / std::max<size_t>(1, tiles)}));
}

// the engine of the tiles and, for chunks of several frames, the engine of the stacked chunk image (false: logged)
bool chunk_engines(int device, int H, int W, size_t chunks, size_t tiles, ebcc_hip_ctx **ctx, ebcc_hip_ctx **rc)
{
    auto none = [] { log_fatal("no MI355X engine available: %s", ebcc_hip_last_error()); return false; };
    *rc = nullptr;
    if (tiles > 1) {
        *rc = get_context(device, (int) (tiles * (size_t) H), W, chunks);
        if (!*rc) return none();
    }
    const int period = tiles > 1 && !tile_geometry_uniform((size_t) H) ? (int) tiles : 1;
    *ctx = get_context(device, H, W, chunks * tiles, period);
    if (!*ctx) return none();
    if (tiles > 1) {                                             // (creating the second engine may have evicted the first)
        *rc = get_context(device, (int) (tiles * (size_t) H), W, chunks);
        if (!*rc) return none();
        std::lock_guard<std::mutex> lock(g_map_mutex);
        if (g_ctx.find(std::make_tuple(device, H, W, period)) == g_ctx.end()) return none();
    }
    return true;
}

// Chunk <-> array copies of the chunking entry points (reference :311-370) as row copies: a chunk is a box, its rows
// are contiguous in the array; rows / frames / columns past the array's edge repeat the last one (index clamping).
struct ChunkBox {
    size_t dims[3], cd[3], cnt[3];
    size_t csize() const { return cd[0] * cd[1] * cd[2]; }
    void origin(size_t cl, size_t org[3]) const { for (int d = 3; d-- > 0;) { org[d] = (cl % cnt[d]) * cd[d]; cl /= cnt[d]; } }
    bool inside(size_t cl) const { size_t o[3]; origin(cl, o); return o[0] + cd[0] <= dims[0] && o[1] + cd[1] <= dims[1] && o[2] + cd[2] <= dims[2]; }
    // chunks that are whole frames of the array: chunk cl is the contiguous range [cl * csize, (cl + 1) * csize)
    bool slabs() const { return cd[1] == dims[1] && cd[2] == dims[2]; }
    void gather(const float *data, size_t cl, float *dst) const
    {
        size_t org[3];
        origin(cl, org);
        const size_t w = std::min(cd[2], dims[2] - org[2]);
        for (size_t z = 0; z < cd[0]; z++) {
            const size_t zi = std::min(org[0] + z, dims[0] - 1);
            for (size_t y = 0; y < cd[1]; y++) {
                const size_t yi = std::min(org[1] + y, dims[1] - 1);
                const float *src = data + (zi * dims[1] + yi) * dims[2] + org[2];
                float *row = dst + (z * cd[1] + y) * cd[2];
                memcpy(row, src, w * sizeof(float));
                for (size_t x = w; x < cd[2]; x++) row[x] = src[w - 1];
            }
        }
    }
    void scatter(const float *src, size_t cl, float *out) const
    {
        size_t org[3];
        origin(cl, org);
        const size_t w = std::min(cd[2], dims[2] - org[2]);
        for (size_t z = 0; z < cd[0] && org[0] + z < dims[0]; z++)
            for (size_t y = 0; y < cd[1] && org[1] + y < dims[1]; y++)
                memcpy(out + ((org[0] + z) * dims[1] + org[1] + y) * dims[2] + org[2], src + (z * cd[1] + y) * cd[2], w * sizeof(float));
    }
};

// Where the chunks of an encode call lie: runs of chunks, each contiguous in (device or host) memory - one run for an
// array, one per frame group unless the groups' arrays happen to follow one another.  The cuts of batches and slices fall
// where they fall: each(lo, cnt, ...) visits the parts of the runs that make up chunks [lo, lo + cnt).
struct FrameSource {
    struct Run { const float *p; size_t first, n; };               // chunks [first, first + n) of the call lie at p
    std::vector<Run> runs;
    size_t total = 0;
    FrameSource() = default;
    FrameSource(const float *p, size_t n) { runs.push_back(Run{p, 0, n}); total = n; }
    void add(const float *p, size_t n, size_t chunk_floats)
    {
        if (!runs.empty() && (uintptr_t) (runs.back().p + runs.back().n * chunk_floats) == (uintptr_t) p) runs.back().n += n;
        else runs.push_back(Run{p, total, n});
        total += n;
    }
    // fn(where, chunk of the batch, chunks) for every run that meets chunks [lo, lo + cnt)
    template <class Fn> void each(size_t lo, size_t cnt, size_t chunk_floats, Fn fn) const
    {
        auto it = std::upper_bound(runs.begin(), runs.end(), lo, [](size_t v, const Run &r) { return v < r.first; });
        for (it = it == runs.begin() ? it : it - 1; it != runs.end() && it->first < lo + cnt; ++it) {
            const size_t a = std::max(lo, it->first), e = std::min(lo + cnt, it->first + it->n);
            if (a < e) fn(it->p + (a - it->first) * chunk_floats, a - lo, e - a);
        }
    }
    // chunks [lo, lo + cnt) where they lie, when one run holds them all (else nullptr)
    const float *in_place(size_t lo, size_t cnt, size_t chunk_floats) const
    {
        const float *at = nullptr;
        size_t parts = 0;
        each(lo, cnt, chunk_floats, [&](const float *p, size_t, size_t) { at = p; parts++; });
        return parts == 1 ? at : nullptr;
    }
};

// ================================================================================================
// slices of a batch
// ================================================================================================
// Slices of a batch: EBCC_HIP_SLICES (encode, 1 = off) / EBCC_HIP_DECODE_SLICES engines of max_frames / slices
// frames each, created on first use.  Small batches stay on the context's own engine.  More than two slices only
// pay when the HIP runtime has a hardware queue for each stream (GPU_MAX_HW_QUEUES, default 4, shared with the
// application's streams; it is read when the runtime starts, so the application sets it): streams that share a
// queue run one after the other.  Default for encode: THREE slices (default_encode_slices below).
// Decode runs as ONE slice since round 2: its launch is as long as the longest SPIHT stream of the batch whatever the
// batch size, and the tier-1 decoder is bound by vector issue slots - two half batches side by side only shared them
// (A/B on one box, tools/gpu/ab_dec.sh: 33 GB/s with one slice, 27 with two).
constexpr size_t kDefaultDecodeSlices = 1;
constexpr size_t kSliceFromFrames = 96;                             // smaller batches run as one slice unless the environment says otherwise
size_t default_encode_slices()
{
    // Four with eight hardware queues in round 1; two at the end of round 2 (the search loops had moved to the device and every
    // further slice repeated the latency-bound launches for fewer frames: 8.4-8.5 GB/s with two, 6.8-7.5 with four); three
    // in round 3 - the probes are cheaper (early exits, leaner fused levels) and the host no longer compresses every prefix,
    // so a third slice finds idle GPU and idle cores again (alternating runs on one box, tools/gpu/host_sweep.sh: 154-160 ms
    // per step with two, 146-153 with three, 160-165 with four).
    return 3;
}
// slices of a batch of n_frames: `k` unless the environment (env_name) says otherwise
size_t slice_count(size_t n_frames, const char *env_name, size_t k)
{
    // (a batch below about a hundred frames is a chain whatever it is cut into - 43 frames of 721 x 1440: 53.9 ms per step as
    //  one slice, 56.8 as two, 60.3 as three; 85 frames: 75.8 / 77.4 / 76.4; 128 frames: 85.9 / 84.6 / 83.0, tools/gpu/slices_frames.sh)
    if (const char *e = getenv(env_name)) k = (size_t) std::max(1L, strtol(e, nullptr, 10));
    else if (n_frames < kSliceFromFrames) k = 1;
    k = std::min<size_t>(k, 8);
    return k < 2 || n_frames < 4 * k ? 1 : k;
}
size_t slice_engines(ebcc_hip_ctx *ctx, size_t n_frames, const char *env_name, size_t k)
{
    k = slice_count(n_frames, env_name, k);
    if (k == 1) return 1;
    const size_t per = (ctx->max_frames + k - 1) / k;
    for (size_t i = 0; i + 1 < k; i++) {                    // slice 0 runs on the context's own engine
        if (i < ctx->lanes.size() && ctx->lanes[i]->max_frames >= per) continue;
        // (a lane made for a finer slicing - encode and decode choose their own - is too small for this one)
        if (i < ctx->lanes.size()) { ebcc_hip_destroy(ctx->lanes[i]); ctx->lanes[i] = nullptr; }
        ebcc_hip_ctx *c = ebcc_hip_create(ctx->device, per, (size_t) ctx->height, (size_t) ctx->width);
        if (i < ctx->lanes.size()) ctx->lanes[i] = c; else if (c) ctx->lanes.push_back(c);
        if (!c) {                                           // out of memory: fall back to the single engine
            ctx->lanes.erase(std::remove(ctx->lanes.begin(), ctx->lanes.end(), (ebcc_hip_ctx *) nullptr), ctx->lanes.end());
            return 1;
        }
    }
    return k;
}

template <class Fn>
int run_slices(ebcc_hip_ctx *ctx, size_t n_frames, Fn fn, const char *env_name, size_t default_slices)
{
    const size_t k = slice_engines(ctx, n_frames, env_name, default_slices);
    if (k == 1) return fn(ctx, (size_t) 0, n_frames, (SliceGate *) nullptr, 1u);
    const size_t per = (n_frames + k - 1) / k;
    const unsigned started = (unsigned) ((n_frames + per - 1) / per);   // (the last slices of a fine slicing can be empty: 8 slices of 33 frames)
    std::vector<int> rc(k, 0);
    std::vector<std::string> err(k);
    std::vector<SliceGate> gates(k);
    std::vector<std::thread> th;
    for (size_t i = 0; i < k; i++) {
        const size_t lo = i * per, hi = std::min(n_frames, lo + per);
        if (lo >= hi) break;
        th.emplace_back([&, i, lo, hi]() {
            // (a thread has its own current device and its own last-error text: the slice reports through rc / err)
            try {
                EBCC_HIP_CHECK(hipSetDevice(ctx->device));
                if (i > 0) gates[i - 1].wait();
                rc[i] = fn(i == 0 ? ctx : ctx->lanes[i - 1], lo, hi - lo, &gates[i], started);
                if (rc[i]) err[i] = ebcc_hip_last_error();
            } catch (const std::exception &e) {
                rc[i] = 1; err[i] = e.what();
                gates[i].release();                                    // (never leave the next slice waiting)
            }
        });
    }
    for (auto &t : th) t.join();
    int worst = 0;
    for (size_t i = 0; i < k; i++) {
        if (rc[i] && !err[i].empty()) set_error("%s", err[i].c_str());
        worst = std::max(worst, rc[i]);
    }
    return worst;
}

// n_frames one-frame chunks as concurrent slices (fc: a config per frame; a slice takes its part of it with its frames)
int run_encode_slices(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const FrameConfig *fc, uint8_t **outs, size_t *sizes,
                      GpuPhase *phase = nullptr)
{
    const size_t n_pix = ctx->n_pix;
    PhaseNote note;
    note.phase = phase;
    struct Over { PhaseNote &n; ~Over() { n.release_once(); } } over{note};                 // (whatever happened to the slices)
    if (phase) phase->acquire();
    return run_slices(ctx, n_frames, [&](ebcc_hip_ctx *c, size_t lo, size_t cnt, SliceGate *next, unsigned slices) {
        note.expect((int) slices);
        return encode_batch(c, d_frames + lo * n_pix, cnt, fc + lo, outs + lo, sizes + lo, next, 1, nullptr, slices, phase ? &note : nullptr);
    }, "EBCC_HIP_SLICES", default_encode_slices());
}

// the decode counterpart (decode overlaps its two layers on the engine's two streams, decode_batch; a second slice hides
// the host side - parsing, zstd, uploads - of one half behind the kernels of the other when there are hardware queues
// for four streams)
// (`region`: d_out holds the output items of these streams; a slice's items are a contiguous part of them, DecodeRegion::part)
int run_decode_slices(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, float *d_out, const DecodeRegion &region = DecodeRegion{})
{
    return run_slices(ctx, n_frames, [&](ebcc_hip_ctx *c, size_t lo, size_t cnt, SliceGate *next, unsigned) {
        size_t first = 0;
        const DecodeRegion part = region.part(lo, cnt, &first);
        return decode_batch(c, streams + lo, sizes + lo, cnt, region.at(d_out, first, ctx->n_pix), next, 1, nullptr, part);
    }, "EBCC_HIP_DECODE_SLICES", kDefaultDecodeSlices);
}

// ================================================================================================
// batches on two alternating engine sets
// ================================================================================================
// The context's engines and a second set of the same size (ebcc_hip_ctx::twin, made on first use), one host thread each.
// Without memory for the second set the first runs every batch; a second set that could not be made is not tried again at
// every call - tens of GB allocated and freed each time - until ebcc_hip_release_second_set / a new context gives the
// memory a chance to have changed.  The schedulers below decide which batch runs where; this owns the second set, the
// threads and the first failure.
struct TwoSets {
    ebcc_hip_ctx *set[2];
    std::atomic<int> worst{0};
    std::string err[2];
    explicit TwoSets(ebcc_hip_ctx *ctx)
    {
        if (!ctx->twin && !ctx->twin_failed) {
            ctx->twin = ebcc_hip_create(ctx->device, ctx->max_frames, (size_t) ctx->height, (size_t) ctx->width);
            if (!ctx->twin) ctx->twin_failed = true;
        }
        set[0] = ctx;
        set[1] = ctx->twin;
    }
    bool failed() const { return worst.load() != 0; }
    void fail(int t, int r, const char *what) { err[t] = what; int e = 0; worst.compare_exchange_strong(e, r); }
    void note(int t, int r) { if (r) fail(t, r, ebcc_hip_last_error()); }          // a batch's status on set t's thread
    // work(t) on set t's thread, with the device current there
    template <class Work> void run(int t, Work &work)
    {
        try {
            EBCC_HIP_CHECK(hipSetDevice(set[0]->device));
            work(t);
        } catch (const std::exception &e) { fail(t, 1, e.what()); }
    }
    // work(1) on a second thread beside work(0) on this one (work(0) alone without a second set)
    template <class Work> void both(Work &work)
    {
        if (!set[1]) { run(0, work); return; }
        std::thread second([&] { run(1, work); });
        run(0, work);
        second.join();
    }
    // the worst status; the first failure's text is this thread's last error
    int status() { if (failed()) set_error("%s", (err[0].empty() ? err[1] : err[0]).c_str()); return worst.load(); }
};

// n_frames one-frame chunks in batches of the context's capacity, alternately on the two sets: one batch at a time is in its
// GPU phase, the next enters it when every slice of the current one has reached its entropy stage (GpuPhase / PhaseNote).
// stage(set, first frame, count) -> where the batch's frames are on the device (a host array is uploaded there: that copy
// runs beside the other batch's kernels too).  fc: a config per frame; a batch takes its part of it with its frames.
// after(set, where, first frame, count, phase), if given, runs on the batch's thread once its streams are made, before the set
// takes its next batch - the frames are still at `where` (the hard-bound loop, harden_batch; its status is the batch's).
template <class Stage, class After = std::nullptr_t>
int encode_batches_alternating(ebcc_hip_ctx *ctx, size_t n_frames, const FrameConfig *fc, uint8_t **outs, size_t *sizes, Stage stage, After after = nullptr)
{
    const size_t cap = ctx->max_frames, batches = (n_frames + cap - 1) / cap;
    auto one_batch = [&](ebcc_hip_ctx *set, const float *where, size_t lo, size_t cnt, GpuPhase *ph) {
        int r = run_encode_slices(set, where, cnt, fc + lo, outs + lo, sizes + lo, ph);
        if constexpr (!std::is_same<After, std::nullptr_t>::value) { if (!r) r = after(set, where, lo, cnt, ph); }
        return r;
    };
    if (batches == 1) return one_batch(ctx, stage(ctx, (size_t) 0, n_frames), 0, n_frames, nullptr);
    TwoSets two(ctx);
    GpuPhase phase;
    std::atomic<size_t> next{0};
    std::mutex redo_m;
    std::vector<size_t> redo;                                        // batches the second set could not stage
    auto work = [&](int t) {
        for (;;) {
            size_t b = next++;
            if (b >= batches) {
                if (t != 0) break;
                std::lock_guard<std::mutex> l(redo_m);
                if (redo.empty()) break;
                b = redo.back(); redo.pop_back();
            }
            if (two.failed()) break;
            const size_t lo = b * cap, cnt = std::min(cap, n_frames - lo);
            const float *where = nullptr;
            try { where = stage(two.set[t], lo, cnt); }
            catch (const std::exception &e) {
                // the second set has no room for its image of the frames: the first set does its batches after its own
                if (t == 0) throw;
                log_warn("second engine set: %s - its batches run on the first", e.what());
                clear_error();
                std::lock_guard<std::mutex> l(redo_m);
                redo.push_back(b);
                for (size_t r = next++; r < batches; r = next++) redo.push_back(r);
                return;
            }
            two.note(t, one_batch(two.set[t], where, lo, cnt, &phase));
        }
    };
    two.both(work);
    if (two.set[1]) two.run(0, work);                               // (what the second set handed back after the first had finished)
    return two.status();
}

// The decode counterpart: both sets free-running on the odd and the even batches - one batch's download (or, for long
// residual streams, its one-wave-per-frame SPIHT chains, which leave most of the chip idle) beside the other's kernels.
//   decode_batches(ctx, n, each)          runs free: each(set, first frame, count) decodes one batch and puts its output where it belongs
//   decode_batches(ctx, n, decode, fold)  ordered: decode(set, first frame, count) -> status, then - in batch order, and only while nothing has failed - fold(same)
// granule: a batch is the context's capacity rounded down to a multiple of it (which must not be 0: the caller refuses a smaller
// context), so the frames that belong together - the x and the y of a step of the pair decode - never fall into different batches.
// Whose turn it is to fold: batch b folds after batch b - 1 has passed its turn on, while the two sets decode side by side.
// A batch passes its turn on when its iteration of the batch loop ends, however it ends (decode_batches: a destructor), every
// batch has an iteration - a loop that has seen a failure goes on and only passes -, and a thread that is left any other way
// (TwoSets::run could not make the device current) says so: await returns when the batch before has passed OR its thread has
// left.  The batches of a thread are in increasing order, so the thread batch b waits for is at a batch below b, which in turn
// waits only for batches this thread is through with: no wait without someone on the way to end it, whatever fails.
struct FoldTurn {
    std::mutex m;
    std::condition_variable cv;
    std::vector<char> passed;
    bool left[2] = {false, false};
    explicit FoldTurn(size_t batches) : passed(batches, 0) {}
    void await(size_t b, int other)
    {
        if (b == 0) return;
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return passed[b - 1] != 0 || left[other]; });
    }
    void pass(size_t b) { { std::lock_guard<std::mutex> l(m); passed[b] = 1; } cv.notify_all(); }
    void leave(int t) { { std::lock_guard<std::mutex> l(m); left[t] = true; } cv.notify_all(); }
};
template <class Decode, class Fold = std::nullptr_t>
int decode_batches(ebcc_hip_ctx *ctx, size_t n, Decode decode, Fold fold = nullptr, size_t granule = 1)
{
    constexpr bool ordered = !std::is_same<Fold, std::nullptr_t>::value;
    const size_t cap = ctx->max_frames / granule * granule, batches = (n + cap - 1) / cap;
    if (batches == 1) {
        const int r = decode(ctx, (size_t) 0, n);
        if constexpr (ordered) { if (!r) fold(ctx, (size_t) 0, n); }
        return r;
    }
    TwoSets two(ctx);
    std::conditional_t<ordered, FoldTurn, size_t> turn(batches);     // (running free: no turns, no condition variable - a number)
    auto work = [&](int t) {
        for (size_t b = (size_t) t; b < batches; b += two.set[1] ? 2 : 1) {
            const size_t lo = b * cap, k = std::min(cap, n - lo);
            if constexpr (!ordered) {
                if (two.failed()) break;
                two.note(t, decode(two.set[t], lo, k));
            } else {
                struct Pass { FoldTurn &turn; size_t b; ~Pass() { turn.pass(b); } } pass{turn, b};      // whatever happens to the batch
                if (two.failed()) continue;
                try {
                    const int r = decode(two.set[t], lo, k);
                    two.note(t, r);
                    if (r) continue;
                    turn.await(b, 1 - t);
                    if (!two.failed()) fold(two.set[t], lo, k);
                } catch (const std::exception &e) { two.fail(t, 1, e.what()); }
            }
        }
    };
    if constexpr (!ordered) two.both(work);
    else if (!two.set[1]) two.run(0, work);
    else {
        std::thread second([&] { two.run(1, work); turn.leave(1); });
        two.run(0, work);
        turn.leave(0);
        second.join();
    }
    return two.status();
}

// n streams decoded, as any reader decodes them, into the set's audit buffer (set->audit, engine.hpp), which is made for `room`
// items of the region: no decoded sample reaches the caller.  -> the status.
int decode_to_audit(ebcc_hip_ctx *set, const uint8_t *const *streams, const size_t *sizes, size_t n, size_t room, const DecodeRegion &region = DecodeRegion{})
{
    float *dec = (float *) set->audit.reserve(room * region.pixels(set->n_pix) * sizeof(float), false, true);
    return run_decode_slices(set, streams, sizes, n, dec, region);
}

// ================================================================================================
// hard error bound: a batch's streams audited on the device, the frames over their bound coded again
// ================================================================================================
// The encoder's bound is soft: it holds on the reconstruction the search looked at, before the mean error is folded into the
// header's min / max (/root/reference/src/ebcc_codec.c:863-868), and a search that could not reach the target only warns.  A
// batch is made hard before its streams leave it (include/ebcc_hip.h): its streams are decoded as any reader decodes them,
// k_frame_errors measures a = max |x - x^| per frame against the frames where the batch read them, and a frame with a > T -
// T: the config's error, times the frame's own range for RELATIVE_ERROR, in float as the encoder multiplies it - is coded
// again with the error e' = (e * (T / a)) * 0.9f, same mode and rate, until it is met, max_rounds re-encodes are spent, or e'
// is 0 or no longer below e.  Only a round's offenders run: their frames as FrameSource runs (adjacent ones where they lie,
// scattered ones copied side by side into the set's offenders buffer), a FrameConfig each.  A frame that ends not met keeps
// the stream of the round with the smallest a, the earliest on ties.  Every stream is what the plain call gives for some error.
constexpr float kHardShrink = 0.9f;                                // (design constants, DESIGN 2.8: with 0.99 a frame can stall)
constexpr int kHardRounds = 6;
struct HardBound { int max_rounds; ebcc_hip_bound_report *report; };           // report: one entry per frame of the call
struct OwnedStreams {                                              // a round's new streams until a frame takes its own over
    std::vector<uint8_t *> p;
    std::vector<size_t> n;
    explicit OwnedStreams(size_t m) : p(m, nullptr), n(m, 0) {}
    ~OwnedStreams() { for (uint8_t *q : p) free(q); }
};
int harden_batch(ebcc_hip_ctx *set, const float *where, size_t cnt, const FrameConfig *fc, uint8_t **outs, size_t *sizes, int max_rounds,
                 ebcc_hip_bound_report *report, GpuPhase *phase)
{
    const size_t n_pix = set->n_pix;
    if (max_rounds <= 0) max_rounds = kHardRounds;
    for (size_t f = 0; f < cnt; f++) report[f] = ebcc_hip_bound_report{INFINITY, 0.0f, fc[f].error, 0, 1};
    if (std::none_of(fc, fc + cnt, [](const FrameConfig &c) { return c.searching(); })) return 0;
    PhaseTimer pt;
    std::vector<ebcc_hip_frame_error> errs(cnt);
    if (const int rc = decode_to_audit(set, outs, sizes, cnt, set->max_frames)) return rc;
    const float *dec = (const float *) set->audit.d;
    frame_errors(set, where, dec, cnt, n_pix, nullptr, errs.data());
    pt.mark("hard bound: audit");
    struct Offender { size_t f; float e; };
    std::vector<Offender> live, next;
    // what a frame over its bound is coded with next; false: it stops as not met
    auto shrink = [](float e, float T, float a, float *to) { *to = (e * (T / a)) * kHardShrink; return *to != 0.0f && *to < e; };
    for (size_t f = 0; f < cnt; f++) {
        ebcc_hip_bound_report &R = report[f];
        R.achieved = errs[f].max_abs;
        if (!fc[f].searching()) continue;
        R.target = fc[f].mode == RELATIVE_ERROR ? fc[f].error * (errs[f].x_max - errs[f].x_min) : fc[f].error;
        R.met = R.achieved <= R.target;
        float e;
        if (!R.met && shrink(fc[f].error, R.target, R.achieved, &e)) live.push_back(Offender{f, e});
    }
    for (int k = 1; !live.empty(); k++, live.swap(next), next.clear()) {
        const size_t m = live.size();
        FrameSource src;
        std::vector<FrameConfig> cfg(m);
        for (size_t i = 0; i < m; i++) {
            src.add(where + live[i].f * n_pix, 1, n_pix);
            cfg[i] = fc[live[i].f];
            cfg[i].error = live[i].e;
        }
        const float *xs = src.in_place(0, m, n_pix);
        if (!xs) {
            float *side = (float *) set->offenders.reserve(m * n_pix * sizeof(float), false, true);
            src.each(0, m, n_pix, [&](const float *p, size_t at, size_t run) {
                EBCC_HIP_CHECK(hipMemcpyAsync(side + at * n_pix, p, run * n_pix * sizeof(float), hipMemcpyDeviceToDevice, set->stream));
            });
            wait_stream(set->stream);
            xs = side;
        }
        OwnedStreams made(m);
        if (const int rc = run_encode_slices(set, xs, m, cfg.data(), made.p.data(), made.n.data(), phase)) return rc;
        if (const int rc = decode_to_audit(set, made.p.data(), made.n.data(), m, set->max_frames)) return rc;
        errs.resize(m);
        frame_errors(set, xs, dec, m, n_pix, nullptr, errs.data());
        for (size_t i = 0; i < m; i++) {
            const size_t f = live[i].f;
            ebcc_hip_bound_report &R = report[f];
            const float a = errs[i].max_abs;
            R.rounds = k;
            if (a < R.achieved) {
                std::swap(outs[f], made.p[i]);                           // (the stream it had is freed with the round's)
                sizes[f] = made.n[i];
                R.achieved = a; R.error_used = live[i].e;
            }
            R.met = a <= R.target;
            float e;
            if (!R.met && k < max_rounds && shrink(live[i].e, R.target, a, &e)) next.push_back(Offender{f, e});
        }
        pt.mark("hard bound: round");
    }
    return 0;
}

// ================================================================================================
// frames in pageable host memory <-> streams
// ================================================================================================
// The chunks of `src` (FrameSource: runs in host memory), `tiles` frames each (tiles > 1: rc is the engine of the stacked chunk
// image), with a config each, in batches of `cap` chunks on ctx.  A batch is uploaded in one go, run after run: uploads issued from inside the slices slow every slice
// down (measured in round 1 with pageable copies, 5.6 against 3.7 GB/s, and again in round 2 through the bounce buffers,
// 7.1 against 6.5).  One-frame chunks in batches that fill the engine run on the alternating sets, anything else batch
// after batch.  0 ok, 1 error, 2 NaN / Inf in the data.
int encode_from_host(ebcc_hip_ctx *ctx, ebcc_hip_ctx *rc, size_t tiles, size_t cap, const FrameSource &src, const FrameConfig *fc,
                     uint8_t **outs, size_t *sizes, const HardBound *hard = nullptr)
{
    const size_t n_pix = ctx->n_pix * tiles, n = src.total;
    PhaseTimer pt[2];                                               // (one per engine set: each has its own thread)
    auto stage = [&](ebcc_hip_ctx *set, size_t lo, size_t cnt) {
        float *d = io_buffer(set, cap * n_pix * sizeof(float));
        src.each(lo, cnt, n_pix, [&](const float *h, size_t at, size_t k) {
            copy_pageable(set, const_cast<float *>(h), d + at * n_pix, k * n_pix * sizeof(float), false);
        });
        pt[set != ctx].mark("host frames: upload");
        return (const float *) d;
    };
    // (hard: the batch is audited against its image in the set's staging buffer, where its offenders are coded again from)
    if (hard) return encode_batches_alternating(ctx, n, fc, outs, sizes, stage, [&](ebcc_hip_ctx *set, const float *where, size_t lo, size_t cnt, GpuPhase *ph) {
        return harden_batch(set, where, cnt, fc + lo, outs + lo, sizes + lo, hard->max_rounds, hard->report + lo, ph);
    });
    if (tiles == 1 && ctx->max_frames == cap) return encode_batches_alternating(ctx, n, fc, outs, sizes, stage);
    for (size_t lo = 0; lo < n; lo += cap) {
        const size_t k = std::min(cap, n - lo);
        const float *d = stage(ctx, lo, k);
        const int r = tiles == 1 ? run_encode_slices(ctx, d, k, fc + lo, outs + lo, sizes + lo)
                                 : encode_batch(ctx, d, k, fc + lo, outs + lo, sizes + lo, nullptr, tiles, rc);
        if (r) return r;
    }
    return 0;
}
// (one array, one config)
int encode_from_host(ebcc_hip_ctx *ctx, ebcc_hip_ctx *rc, size_t tiles, size_t cap, const float *data, size_t n, const codec_config_t *cfg,
                     uint8_t **outs, size_t *sizes)
{
    const std::vector<FrameConfig> fc(n, FrameConfig(*cfg));
    return encode_from_host(ctx, rc, tiles, cap, FrameSource(data, n), fc.data(), outs, sizes);
}

// The decode counterpart: streams of n chunks -> host memory at `out`, one download per batch (copies issued from inside
// the slices slowed them down).  `prefault`: host threads are mapping the pages of `out`, joined before the first download.
// Chunks of several frames are one decode_batch per batch: the slice engines have no tile geometry.
// `region`: `out` holds its output items, and only they cross to the host; a window's items of a batch are a contiguous part of
// them.  A list: a batch's boxes lie compact in the device image, one behind the other at pitch `cols` (ListStage), and cross
// as one download - straight to their place where they lie in `out` the same way, as the boxes of a compact
// [n_boxes][rows][cols] array do, else into a host image of the same layout, from which they are put into their rectangles of
// `out` row by row.  Nothing else of `out` is touched.
struct ListStage {
    std::vector<ebcc_hip_placed_box> boxes;
    size_t floats = 0;
    bool in_place = true;                                            // the staged layout is that of `out` from list[0].out_offset on
    ListStage(const ebcc_hip_placed_box *list, size_t n) : boxes(list, list + n)
    {
        for (ebcc_hip_placed_box &b : boxes) {
            in_place = in_place && b.out_pitch == b.cols && b.out_offset == list[0].out_offset + floats;
            b.out_offset = floats; b.out_pitch = b.cols; floats += b.rows * b.cols;
        }
    }
    void place(const ebcc_hip_placed_box *list, const float *image, float *out) const
    {
        for (size_t e = 0; e < boxes.size(); e++)
            for (size_t y = 0; y < list[e].rows; y++)
                memcpy(out + list[e].out_offset + y * list[e].out_pitch, image + boxes[e].out_offset + y * boxes[e].cols, list[e].cols * sizeof(float));
    }
};
int decode_to_host(ebcc_hip_ctx *ctx, ebcc_hip_ctx *rc, size_t tiles, size_t cap, const uint8_t *const *streams, const size_t *sizes, size_t n,
                   float *out, Prefault *prefault, const DecodeRegion &region = DecodeRegion{})
{
    const size_t n_pix = region.pixels(ctx->n_pix * tiles);
    auto one_batch = [&](ebcc_hip_ctx *set, size_t lo, size_t k) {
        PhaseTimer pt;
        size_t first = 0;
        const DecodeRegion part = region.part(lo, k, &first);
        if (part.kind == DecodeRegion::List) {
            if (part.n == 0) return 0;
            const ListStage stage(part.list, part.n);
            DecodeRegion staged = part;
            staged.list = stage.boxes.data(); staged.out_floats = stage.floats;
            float *d = io_buffer(set, stage.floats * sizeof(float));
            pt.mark("host decode: device image");
            const int r = run_decode_slices(set, streams + lo, sizes + lo, k, d, staged);
            if (r) return r;
            pt.mark("host decode: decode");
            if (prefault) prefault->join();
            pt.mark("host decode: output pages");
            if (stage.in_place) copy_pageable(set, out + part.list[0].out_offset, d, stage.floats * sizeof(float), true);
            else {
                std::vector<float> image(stage.floats);
                copy_pageable(set, image.data(), d, stage.floats * sizeof(float), true);
                stage.place(part.list, image.data(), out);
            }
            pt.mark("host decode: download");
            return 0;
        }
        float *d = io_buffer(set, cap * n_pix * sizeof(float));
        pt.mark("host decode: device image");
        const int r = tiles > 1 ? decode_batch(set, streams + lo, sizes + lo, k, d, nullptr, tiles, rc, part)
                                : run_decode_slices(set, streams + lo, sizes + lo, k, d, part);
        if (r) return r;
        pt.mark("host decode: decode");
        if (prefault) prefault->join();
        pt.mark("host decode: output pages");
        copy_pageable(set, out + first * n_pix, d, k * n_pix * sizeof(float), true);
        pt.mark("host decode: download");
        return 0;
    };
    if (tiles == 1 && ctx->max_frames == cap) return decode_batches(ctx, n, one_batch);
    for (size_t lo = 0; lo < n; lo += cap) {
        const int r = one_batch(ctx, lo, std::min(cap, n - lo));
        if (r) return r;
    }
    return 0;
}

// The reference-compatible entry points' host arrays on the engines cached for `device`: n chunks of `tiles` frames of
// H x W each.  Returns 0 ok, 1 error (logged), 2 NaN / Inf in the data (the caller exits as the reference does,
// /root/reference/src/ebcc_codec.c:598-605).
int encode_on_device(int device, const float *data, size_t n, int H, int W, const codec_config_t *cfg, uint8_t **outs, size_t *sizes,
                     size_t tiles = 1)
{
    return on_codec(device, 1, [&] {
        const size_t cap = std::min(n, batch_capacity((size_t) H * W * tiles, tiles));
        ebcc_hip_ctx *ctx = nullptr, *rc = nullptr;
        PhaseTimer pt;
        if (!chunk_engines(device, H, W, cap, tiles, &ctx, &rc)) return 1;
        pt.mark("host frames: engine");
        return encode_from_host(ctx, rc, tiles, cap, data, n, cfg, outs, sizes);
    });
}

// A list of independent chunks spread over the devices of device_list(): contiguous blocks, one host thread per device
// (/root/reference/src/ebcc_codec.c:1007-1046 is a serial loop over the chunks; the order of the results is that of the
// chunks).  fn(device, first, count) -> status; returns the worst status.
template <class Fn>
int run_on_devices(size_t n_chunks, Fn fn)
{
    std::vector<int> devs = device_list();
    if (devs.size() > n_chunks) devs.resize(std::max<size_t>(1, n_chunks));
    if (devs.size() == 1) return fn(devs[0], (size_t) 0, n_chunks);
    const size_t per = (n_chunks + devs.size() - 1) / devs.size();
    std::vector<int> rc(devs.size(), 0);
    std::vector<std::thread> th;
    for (size_t i = 0; i < devs.size(); i++) {
        const size_t lo = i * per, hi = std::min(n_chunks, lo + per);
        if (lo >= hi) break;
        th.emplace_back([&, i, lo, hi]() { rc[i] = fn(devs[i], lo, hi - lo); });
    }
    for (auto &t : th) t.join();
    int worst = 0;
    for (int r : rc) worst = std::max(worst, r);
    return worst;
}

// ================================================================================================
// what the batch entry points of a caller's context share
// ================================================================================================
// Encode: the argument checks, out_streams emptied first and, when the call fails, every stream made so far freed again;
// code() runs in the device prologue and returns the status.
template <class Code>
int encode_checked(ebcc_hip_ctx *ctx, size_t n, uint8_t **outs, size_t *sizes, Code &&code)
{
    log_set_level_from_env();
    for (size_t f = 0; f < n; f++) { outs[f] = nullptr; sizes[f] = 0; }
    const int rc = on_codec(ctx->device, 1, code);
    if (rc)
        for (size_t f = 0; f < n; f++) { free(outs[f]); outs[f] = nullptr; sizes[f] = 0; }
    return rc;
}
template <class Code>
int encode_call(const char *who, ebcc_hip_ctx *ctx, const void *frames, size_t n, const codec_config_t *cfg, uint8_t **outs, size_t *sizes,
                Code &&code)
{
    if (!ctx || !frames || !cfg || !outs || !sizes || n < 1) { set_error("%s: bad arguments", who); return 1; }
    if (cfg->dims[0] != 1 || (int) cfg->dims[1] != ctx->height || (int) cfg->dims[2] != ctx->width) {
        set_error("%s: config dims must be (1, %d, %d)", who, ctx->height, ctx->width);
        return 1;
    }
    return encode_checked(ctx, n, outs, sizes, code);
}

// Device-resident frames: batches of the context's capacity on the alternating sets (one batch: one run_encode_slices).  A
// batch whose frames are adjacent in memory is coded where it lies; otherwise its runs are brought into the engine set's
// staging buffer, one device-to-device copy per run on that set's stream, and the stage waits for them (the slices read
// them on streams of their own) - as the container stage does with the chunks it gathers.
int encode_device_frames(ebcc_hip_ctx *ctx, const FrameSource &src, const FrameConfig *fc, uint8_t **outs, size_t *sizes, const HardBound *hard = nullptr)
{
    const size_t n_pix = ctx->n_pix, cap = std::min(src.total, ctx->max_frames);
    PhaseTimer pt[2];
    auto stage = [&](ebcc_hip_ctx *set, size_t lo, size_t cnt) {
        if (const float *where = src.in_place(lo, cnt, n_pix)) return where;
        float *d = io_buffer(set, cap * n_pix * sizeof(float));
        src.each(lo, cnt, n_pix, [&](const float *p, size_t at, size_t k) {
            EBCC_HIP_CHECK(hipMemcpyAsync(d + at * n_pix, p, k * n_pix * sizeof(float), hipMemcpyDeviceToDevice, set->stream));
        });
        wait_stream(set->stream);
        pt[set != ctx].mark("frame groups: runs copied");
        return (const float *) d;
    };
    if (!hard) return encode_batches_alternating(ctx, src.total, fc, outs, sizes, stage);
    return encode_batches_alternating(ctx, src.total, fc, outs, sizes, stage, [&](ebcc_hip_ctx *set, const float *where, size_t lo, size_t cnt, GpuPhase *ph) {
        return harden_batch(set, where, cnt, fc + lo, outs + lo, sizes + lo, hard->max_rounds, hard->report + lo, ph);
    });
}
int encode_resident(const char *who, ebcc_hip_ctx *ctx, const float *d_frames, size_t n, const codec_config_t *cfg, uint8_t **outs, size_t *sizes)
{
    return encode_call(who, ctx, d_frames, n, cfg, outs, sizes, [&] {
        const std::vector<FrameConfig> fc(n, FrameConfig(*cfg));
        return encode_device_frames(ctx, FrameSource(d_frames, n), fc.data(), outs, sizes);
    });
}
// ---- frame groups (include/ebcc_hip.h): arrays of frames with a config each, coded as one call
// What ebcc_hip_groups_check checks, for frames of height x width: the total number of frames, or -1 with the message set.
long groups_total(const char *who, size_t height, size_t width, const ebcc_hip_frame_group *groups, size_t n_groups)
{
    if (!groups || n_groups < 1) { set_error("%s: no groups", who); return -1; }
    if (height < 1 || width < 1 || height > 2047 || width > 2047) { set_error("%s: unsupported geometry %zu x %zu", who, height, width); return -1; }
    size_t total = 0, bytes = 0;
    for (size_t g = 0; g < n_groups; g++) {
        const ebcc_hip_frame_group &G = groups[g];
        if (!G.frames || G.n_frames < 1) { set_error("%s: group %zu has no frames", who, g); return -1; }
        if ((uintptr_t) G.frames & 3) { set_error("%s: the frames of group %zu are not 4-byte aligned", who, g); return -1; }
        if (G.config.dims[0] != 1 || G.config.dims[1] != height || G.config.dims[2] != width) {
            set_error("%s: group %zu: config dims (%zu, %zu, %zu) are not (1, %zu, %zu)", who, g, G.config.dims[0], G.config.dims[1], G.config.dims[2], height, width);
            return -1;
        }
        if (__builtin_add_overflow(total, G.n_frames, &total) || total > (size_t) LONG_MAX ||
            __builtin_mul_overflow(total, height * width * sizeof(float), &bytes)) {
            set_error("%s: the number of frames overflows at group %zu", who, g);
            return -1;
        }
    }
    return (long) total;
}

enum class GroupForm { Frames, Shard, Host };
// The three encode entry points: the check, the context, the capacity (frames form); then, in the device prologue, the ranges
// of the groups whose bound is relative to the range of the whole group - one launch and one wait for all of them (device
// forms), a scan on the host pool (host form: nothing extra is uploaded) - restated as MAX_ERROR with error * (max - min) in
// host float arithmetic as ebcc_encode_chunking_compat does (:1078-1087), and the frames of all groups as one list with a
// config each.  NaN / Inf: 2 with the group named - before anything is coded for a group range, else when a batch meets it.
// hard: the batches are made hard (harden_batch) and the call returns 3 when every frame is coded but some are not met.
int encode_groups(const char *who, ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, uint8_t **outs, size_t *sizes,
                  GroupForm form, const HardBound *hard = nullptr)
{
    if (!ctx || !outs || !sizes) { set_error("%s: bad arguments", who); return 1; }
    if (ctx->tile_period != 1) { set_error("%s: the context is one for chunks of several frames", who); return 1; }
    const long checked = groups_total(who, (size_t) ctx->height, (size_t) ctx->width, groups, n_groups);
    if (checked < 0) return 1;
    const size_t total = (size_t) checked, n_pix = ctx->n_pix;
    if (form == GroupForm::Frames && total > ctx->max_frames) {
        for (size_t f = 0; f < total; f++) { outs[f] = nullptr; sizes[f] = 0; }
        set_error("%s: %zu frames, the context holds %zu", who, total, ctx->max_frames);
        return 1;
    }
    std::vector<FrameConfig> fc;
    fc.reserve(total);
    FrameSource src;
    std::vector<size_t> first(n_groups), ranged, all(n_groups);
    for (size_t g = 0; g < n_groups; g++) {
        const ebcc_hip_frame_group &G = groups[g];
        first[g] = fc.size(); all[g] = g;
        fc.insert(fc.end(), G.n_frames, FrameConfig(G.config));
        src.add(G.frames, G.n_frames, n_pix);
        if (G.range_of_group && G.config.residual_compression_type == RELATIVE_ERROR) ranged.push_back(g);
    }
    auto range_keys = [&](const std::vector<size_t> &list) {
        std::vector<const float *> ptrs;
        std::vector<size_t> lens;
        for (size_t g : list) { ptrs.push_back(groups[g].frames); lens.push_back(groups[g].n_frames * n_pix); }
        std::vector<unsigned> keys(3 * list.size());
        if (form == GroupForm::Host) host_range_keys(ptrs.data(), lens.data(), list.size(), keys.data());
        else group_range_keys(ctx, ptrs.data(), lens.data(), list.size(), keys.data());
        return keys;
    };
    auto nonfinite = [&](size_t g) {
        log_fatal("NaN or Inf found in data of group %zu", g);
        set_error("%s: NaN or Inf found in the data of group %zu", who, g);
        return 2;
    };
    std::vector<ebcc_hip_bound_report> own_report;
    HardBound bound{0, nullptr};
    if (hard) {
        bound = *hard;
        if (!bound.report) { own_report.resize(total); bound.report = own_report.data(); }
        hard = &bound;
    }
    const int status = encode_checked(ctx, total, outs, sizes, [&] {
        if (!ranged.empty()) {
            const std::vector<unsigned> keys = range_keys(ranged);
            for (size_t i = 0; i < ranged.size(); i++) if (keys[3 * i + 2]) return nonfinite(ranged[i]);
            for (size_t i = 0; i < ranged.size(); i++) {
                const ebcc_hip_frame_group &G = groups[ranged[i]];
                FrameConfig c(G.config);
                c.error *= float_of_order_key(keys[3 * i + 1]) - float_of_order_key(keys[3 * i]);
                c.mode = MAX_ERROR;
                std::fill_n(fc.begin() + first[ranged[i]], G.n_frames, c);
            }
        }
        const int rc = form == GroupForm::Host ? encode_from_host(ctx, nullptr, 1, ctx->max_frames, src, fc.data(), outs, sizes, hard)
                                               : encode_device_frames(ctx, src, fc.data(), outs, sizes, hard);
        if (rc == 2) {                                              // (a batch met it: which group was it)
            const std::vector<unsigned> keys = range_keys(all);
            for (size_t g = 0; g < n_groups; g++) if (keys[3 * g + 2]) return nonfinite(g);
            set_error("%s: NaN or Inf found in the data", who);
        }
        return rc;
    });
    if (status || !hard) return status;
    const size_t missed = (size_t) std::count_if(bound.report, bound.report + total, [](const ebcc_hip_bound_report &r) { return !r.met; });
    if (missed) { set_error("%s: %zu of %zu frames are coded but not within their bound", who, missed, total); return 3; }
    return 0;
}

// The list of a list entry point, as the call it stands for: the streams of the frames the boxes name, in their order, with the
// boxes' frames counted over those.  A frame no box names is not looked at - not even its pointer.
struct BoxCall {
    std::vector<const uint8_t *> streams;
    std::vector<size_t> sizes;
    std::vector<ebcc_hip_placed_box> list;
};

// The decode entry points: `region` as the caller states it, and the checks in their order - bad batch (`one_batch`, the _frames
// forms: at most the context's capacity of frames), bad arguments, a window or a list that does not fit the context's frames
// (nothing is written for one that is refused) - then run(region, streams, sizes, n) in the device prologue.
// (decode_region: the checks of the region alone, which also turn a list into its BoxCall - for a caller that holds the device;
// decode_call with `held`: the caller holds the device's lock and has made the device current - run() runs where it stands, and
// what it throws is the caller's prologue's to catch)
int decode_region(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *&streams, const size_t *&sizes, size_t &n_frames, DecodeRegion &region,
                  BoxCall &call)
{
    if (region.kind == DecodeRegion::Window) {
        const size_t H = (size_t) ctx->height, W = (size_t) ctx->width, row0 = region.row0, col0 = region.col0, rows = region.rows, cols = region.cols;
        if (rows < 1 || cols < 1 || row0 >= H || col0 >= W || rows > H - row0 || cols > W - col0) {
            set_error("%s: the window [%zu, +%zu) x [%zu, +%zu) is empty or not inside the %zu x %zu frame", who, row0, rows, col0, cols, H, W);
            return 1;
        }
    } else if (region.kind == DecodeRegion::List) {
        if (ctx->tile_period != 1) { set_error("%s: chunks of several frames are not supported", who); return 1; }
        if (!j2k_list_check(who, static_cast<const J2kBuffers *>(ctx->j2k)->geom, n_frames, region.list, region.n, region.out_floats)) return 1;
        call.list.assign(region.list, region.list + region.n);
        for (size_t e = 0; e < region.n; e++) {
            const size_t f = region.list[e].frame;
            if (e == 0 || f != region.list[e - 1].frame) { call.streams.push_back(streams[f]); call.sizes.push_back(sizes[f]); }
            call.list[e].frame = call.streams.size() - 1;
        }
        region.list = call.list.data();
        streams = call.streams.data(); sizes = call.sizes.data(); n_frames = call.streams.size();
    }
    return 0;
}
template <class Run>
int decode_call(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const void *out,
                DecodeRegion region, bool one_batch, Run &&run, bool held = false)
{
    if (one_batch && (!ctx || n_frames < 1 || n_frames > ctx->max_frames)) { set_error("%s: bad batch", who); return 1; }
    if (!ctx || !streams || !sizes || !out || n_frames < 1) { set_error("%s: bad arguments", who); return 1; }
    BoxCall call;
    if (decode_region(who, ctx, streams, sizes, n_frames, region, call)) return 1;
    if (held) return run(region, streams, sizes, n_frames);
    return on_codec(ctx->device, 1, [&] { return run(region, streams, sizes, n_frames); });
}
// device output: batches of the context's capacity on the two sets side by side, each as its slices
int decode_resident(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, float *d_out,
                    const DecodeRegion &asked, bool one_batch)
{
    return decode_call(who, ctx, streams, sizes, n_frames, d_out, asked, one_batch, [&](const DecodeRegion &region, const uint8_t *const *st, const size_t *sz, size_t n) {
        return decode_batches(ctx, n, [&](ebcc_hip_ctx *set, size_t lo, size_t k) {
            size_t first = 0;
            const DecodeRegion part = region.part(lo, k, &first);
            return run_decode_slices(set, st + lo, sz + lo, k, region.at(d_out, first, ctx->n_pix), part);
        });
    });
}
// host output.  own_output: the output array is the call's to fill whole - frames, windows, the compact array of a _boxes entry
// point - and its pages are mapped while the GPU decodes; else (placed boxes) it is not the call's to clear, and no page of it
// is touched ahead of the boxes.  The entry point says which: the list does not.
int decode_host(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, float *h_out, const DecodeRegion &asked,
                bool own_output = true)
{
    return decode_call(who, ctx, streams, sizes, n_frames, h_out, asked, false, [&](const DecodeRegion &region, const uint8_t *const *st, const size_t *sz, size_t n) {
        const size_t floats = region.kind == DecodeRegion::List ? region.out_floats : n * region.pixels(ctx->n_pix);
        Prefault prefault(h_out, own_output ? floats * sizeof(float) : 0);
        return decode_to_host(ctx, nullptr, 1, ctx->max_frames, st, sz, n, h_out, &prefault, region);
    });
}

// The _boxes entry points: the placed list in which box e lies at index e of a compact [n_boxes][rows][cols] array
// (j2k_boxes_as_placed), which is the call's to fill whole.
int decode_boxes(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_box *boxes,
                 size_t n_boxes, size_t rows, size_t cols, float *out, bool host, bool one_batch)
{
    std::vector<ebcc_hip_placed_box> placed;
    size_t out_floats = 0;
    if (!j2k_boxes_as_placed(who, boxes, n_boxes, rows, cols, placed, &out_floats)) return 1;
    const DecodeRegion region = DecodeRegion::placed_list(placed.data(), placed.size(), out_floats);
    return host ? decode_host(who, ctx, streams, sizes, n_frames, out, region) : decode_resident(who, ctx, streams, sizes, n_frames, out, region, one_batch);
}

// ---- consumers of decoded frames (audit, reduce decode, area series, regrid decode, quantile decode, time-map decode, pair decode, spell decode).  What one asks the driver for, its own arguments checked:
struct DecodedAsk {
    const uint8_t *const *streams = nullptr;
    const size_t *sizes = nullptr, *names = nullptr;   // names[i]: the number stream i has in the caller's list, for a message (null: i)
    size_t n = 0;
    const void *out = nullptr;              // what the caller gave for the results: must not be null
    ebcc_hip_region box{};                  // what is decoded of every frame: a window, or the frame when the box is the frame
    bool parsed_first = false;              // every stream must parse as a frame stream before anything is written
    const char *decode_mark = "";           // EBCC_HIP_PHASE_TIMING label of a batch's decode
    std::function<bool()> ready;            // if set: runs in the device prologue before the first decode; false: refused, message set
    size_t granule = 1;                     // streams that must share a batch: n is a multiple, the context's capacity at least one (decode_batches)
};
// The one driver: the refusals of the context, ask(DecodedAsk &) -> false when the consumer refuses its own arguments (message
// set), the pre-parse, decode_call's checks and device prologue, then the batches of the context's capacity on the two sets
// (decode_batches), each decoded into its set's audit buffer and handed to per_batch(set, decoded, first stream, count, timer) -
// free-running, or `ordered`: in batch order and only while nothing has failed.  one_batch: at most the context's capacity.
// held: the caller is inside on_codec for the context's device (a consumer of several passes keeps the lock over all of them).
template <class Ask, class PerBatch>
int consume_decoded(const char *who, ebcc_hip_ctx *ctx, bool one_batch, bool ordered, Ask ask, PerBatch per_batch, bool held = false)
{
    if (!ctx) { set_error(one_batch ? "%s: bad batch" : "%s: bad arguments", who); return 1; }
    if (ctx->tile_period != 1) { set_error("%s: the context is one for chunks of several frames", who); return 1; }
    DecodedAsk a;
    if (!ask(a)) return 1;
    if (a.parsed_first)
        for (size_t i = 0; i < a.n; i++) {
            ParsedFrame pf;
            if (!a.streams[i] || !parse_frame(a.streams[i], a.sizes[i], pf)) { set_error("%s: frame %zu: not a frame stream", who, a.names ? a.names[i] : i); return 1; }
        }
    const bool whole = a.box.rows == (size_t) ctx->height && a.box.cols == (size_t) ctx->width;
    const DecodeRegion asked = whole ? DecodeRegion{} : DecodeRegion::window(a.box.row0, a.box.col0, a.box.rows, a.box.cols);
    return decode_call(who, ctx, a.streams, a.sizes, a.n, a.out, asked, one_batch, [&](const DecodeRegion &region, const uint8_t *const *sp, const size_t *zp, size_t n) {
        if (a.ready && !a.ready()) return 1;
        const size_t room = std::min(n, ctx->max_frames);
        PhaseTimer pt[2];                                               // (one per engine set: each has its own thread)
        auto decode = [&](ebcc_hip_ctx *set, size_t lo, size_t k) {
            const int r = decode_to_audit(set, sp + lo, zp + lo, k, room, region);
            pt[set != ctx].mark(a.decode_mark);
            return r;
        };
        auto hand = [&](ebcc_hip_ctx *set, size_t lo, size_t k) { per_batch(set, (const float *) set->audit.d, lo, k, pt[set != ctx]); };
        if (ordered) return decode_batches(ctx, n, decode, hand, a.granule);
        return decode_batches(ctx, n, [&](ebcc_hip_ctx *set, size_t lo, size_t k) {
            if (const int r = decode(set, lo, k)) return r;
            hand(set, lo, k);
            return 0;
        }, nullptr, a.granule);
    }, held);
}

// ---- audit: the error of what the streams decode to, against the originals, measured on the device
// k_frame_errors takes each batch against the originals: where they lie on the device, or uploaded batch by batch into the
// set's staging buffer.  NaN / Inf in the originals: the other frames are still reported, the call returns 2.
enum class AuditForm { Frames, Shard, Host };
int audit(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const float *originals,
          const float *bound, ebcc_hip_frame_error *report, AuditForm form)
{
    std::atomic<int> nonfinite{0};
    const int rc = consume_decoded(who, ctx, form == AuditForm::Frames, false, [&](DecodedAsk &a) {
        if (!report || ((uintptr_t) originals & 3)) { set_error("%s: bad arguments", who); return false; }
        a.streams = streams; a.sizes = sizes; a.n = n_frames; a.out = originals;
        a.box = ebcc_hip_region{0, 0, (size_t) ctx->height, (size_t) ctx->width};
        a.decode_mark = "audit: decode";
        return true;
    }, [&](ebcc_hip_ctx *set, const float *decoded, size_t lo, size_t k, PhaseTimer &pt) {
        const size_t n_pix = ctx->n_pix;
        const float *x = originals + lo * n_pix;
        if (form == AuditForm::Host) {
            float *up = io_buffer(set, std::min(n_frames, ctx->max_frames) * n_pix * sizeof(float));
            copy_pageable(set, const_cast<float *>(x), up, k * n_pix * sizeof(float), false);
            pt.mark("audit: upload");
            x = up;
        }
        if (frame_errors(set, x, decoded, k, n_pix, bound ? bound + lo : nullptr, report + lo) == 2) nonfinite = 1;
        pt.mark("audit: statistics");
    });
    if (!rc && nonfinite.load()) { set_error("%s: NaN or Inf found in the originals", who); return 2; }
    return rc;
}

// ---- the named steps of a binned call, as the decode sees them: streams and sizes (one to a step, or an x and a y), the step's
// number in the caller's list and its bin.  per_step(t, bin) adds the streams of step t and what else the consumer keeps of it
// -> 1, or 0: the step is left out, or -1: refused, the message set.
struct NamedSteps {
    std::vector<const uint8_t *> st;
    std::vector<size_t> sz, names;
    std::vector<uint32_t> bn;
    void add(const uint8_t *stream, size_t size) { st.push_back(stream); sz.push_back(size); }
    template <class PerStep> bool fill(size_t n, const uint32_t *bin, PerStep per_step)
    {
        for (size_t t = 0; t < n; t++) {
            const uint32_t b = bin ? bin[t] : 0u;
            if (b == EBCC_HIP_NO_BIN) continue;
            const int taken = per_step(t, b);
            if (taken < 0) return false;
            if (taken) { bn.push_back(b); names.push_back(t); }
        }
        return true;
    }
    void ask(DecodedAsk &a) const { a.streams = st.data(); a.sizes = sz.data(); a.n = st.size(); }
    void add_counts(uint64_t *count) const { for (const uint32_t b : bn) count[b]++; }
};

// ---- reduce decode: statistics over time from the streams (include/ebcc_hip.h: ebcc_hip_time_stats; k_time_fold, array_stats.hip)
// The named frames are the call the decode sees; the fold is ordered: a bin's additions are in frame order.
int reduce_shard(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin,
                 size_t row0, size_t col0, const ebcc_hip_time_stats *stats)
{
    NamedSteps ns;
    const int rc = consume_decoded(who, ctx, false, true, [&](DecodedAsk &a) {
        if (time_stats_named(who, (size_t) ctx->height, (size_t) ctx->width, stats, bin, n_frames, row0, col0) < 0) return false;
        if (!streams || !sizes) { set_error("%s: bad arguments", who); return false; }
        ns.fill(n_frames, bin, [&](size_t f, uint32_t) { ns.add(streams[f], sizes[f]); return 1; });
        ns.ask(a);
        a.names = ns.names.data(); a.out = stats;
        a.box = ebcc_hip_region{row0, col0, stats->rows, stats->cols};
        a.parsed_first = true;
        a.decode_mark = "reduce: decode";
        return true;
    }, [&](ebcc_hip_ctx *set, const float *decoded, size_t lo, size_t k, PhaseTimer &pt) {
        time_fold(set, decoded, k, stats->rows * stats->cols, ns.bn.data() + lo, *stats);
        pt.mark("reduce: fold");
    });
    if (!rc) ns.add_counts(stats->count);
    return rc;
}

// ---- area series: statistics over a region at every time step (include/ebcc_hip.h: ebcc_hip_area_spec; k_area_rows, array_stats.hip)
// The bounding box of the regions is what is decoded, and every batch is folded where it was decoded and writes its own rows of
// `out`: batches never meet, so the two sets run free.  The weights are looked at once, on the first set, before any decode.
int series_shard(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_area_spec *spec,
                 ebcc_hip_area_stat *out)
{
    ebcc_hip_region bb{};
    return consume_decoded(who, ctx, false, false, [&](DecodedAsk &a) {
        const size_t H = (size_t) ctx->height, W = (size_t) ctx->width;
        if (area_checked(who, H, W, spec, &bb) < 0) return false;
        size_t bytes = 0;
        if (!streams || !sizes || !out || n_frames < 1) { set_error("%s: bad arguments", who); return false; }
        if (__builtin_mul_overflow(n_frames, spec->n_regions, &bytes) || __builtin_mul_overflow(bytes, sizeof(ebcc_hip_area_stat), &bytes)) {
            set_error("%s: the size of the records overflows", who);
            return false;
        }
        a.streams = streams; a.sizes = sizes; a.n = n_frames; a.out = out;
        a.box = bb;
        a.parsed_first = true;
        a.decode_mark = "series: decode";
        a.ready = [&, W] {
            if (spec->d_w_pix && area_weights_bad(ctx, spec->d_w_pix, W, bb)) { set_error("%s: d_w_pix holds a negative value, a NaN or an Inf", who); return false; }
            return true;
        };
        return true;
    }, [&](ebcc_hip_ctx *set, const float *decoded, size_t lo, size_t k, PhaseTimer &pt) {
        area_fold(set, AreaItems{decoded, bb.rows * bb.cols, (unsigned) bb.cols, (unsigned) bb.row0, (unsigned) bb.col0}, k, (size_t) ctx->height, (size_t) ctx->width,
                  *spec, out + lo * spec->n_regions);
        pt.mark("series: fold");
    });
}

// ---- regrid decode: the same fields on another grid (include/ebcc_hip.h: ebcc_hip_regrid_spec; k_regrid, regrid.hip)
// The bounding box of the supports is what is decoded, and every batch is resampled where it was decoded and writes its own
// frames of the output: batches never meet, so the two sets run free.  The tables go up once per engine set, ahead of the set's
// first batch (the window and the full decode keep no table of their own in set->boxes).  host: the output is pageable host
// memory - a batch is resampled into the set's device image (io) and only that crosses PCIe.
int regrid_shard(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_regrid_spec *spec,
                 float *out, bool host)
{
    ebcc_hip_region bb{};
    size_t out_pix = 0;
    bool up[2] = {false, false};
    return consume_decoded(who, ctx, false, false, [&](DecodedAsk &a) {
        const long checked = regrid_checked(who, (size_t) ctx->height, (size_t) ctx->width, spec, &bb);
        if (checked < 0) return false;
        out_pix = (size_t) checked;
        size_t bytes = 0;
        if (!streams || !sizes || !out || ((uintptr_t) out & 3) || n_frames < 1) { set_error("%s: bad arguments", who); return false; }
        if (__builtin_mul_overflow(n_frames, out_pix * sizeof(float), &bytes)) { set_error("%s: the size of the output overflows", who); return false; }
        a.streams = streams; a.sizes = sizes; a.n = n_frames; a.out = out;
        a.box = bb;
        a.parsed_first = true;
        a.decode_mark = "regrid: decode";
        return true;
    }, [&](ebcc_hip_ctx *set, const float *decoded, size_t lo, size_t k, PhaseTimer &pt) {
        bool &sent = up[set != ctx];
        if (!sent) { regrid_upload(set, *spec, bb); sent = true; }
        float *const d = host ? io_buffer(set, std::min(n_frames, ctx->max_frames) * out_pix * sizeof(float)) : out + lo * out_pix;
        regrid_items(set, RegridItems{decoded, bb.rows * bb.cols, (unsigned) bb.cols, (unsigned) bb.row0, (unsigned) bb.col0}, k, (size_t) ctx->width, *spec, d);
        if (host) copy_pageable(set, out + lo * out_pix, d, k * out_pix * sizeof(float), true);
        pt.mark("regrid: map");
    });
}

// ---- quantile decode: order statistics over time per pixel (include/ebcc_hip.h: ebcc_hip_time_ranks; k_rank_count, quantile.hip)
// A radix select over the series: kRankPasses passes, each one ordered consume_decoded call over the frames that are read - the
// counters are shared between the batches, which count in their turns - and after each the advance on the calling thread.  The
// state of the select lives in the context (ctx->ranks) from the first pass to the last, so the device's lock is taken once and
// held over all of them (consume_decoded's `held`): calls of several threads on one context run one after the other, as every
// other entry point's do.  The check, the compaction and the parse belong to the first pass, which also sets the workspace;
// d_out and count are written after the last pass, so a refusal or a damaged stream in any pass leaves both untouched.  A frame
// whose bin has no slot in use is counted and not read.
int quantile_shard(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin,
                   size_t row0, size_t col0, const ebcc_hip_time_ranks *spec)
{
    if (!ctx) { set_error("%s: bad arguments", who); return 1; }
    NamedSteps ns;
    RankPlan plan;
    return on_codec(ctx->device, 1, [&] {
        for (int pass = 0; pass < kRankPasses; pass++) {
            const int rc = consume_decoded(who, ctx, false, true, [&](DecodedAsk &a) {
                if (pass == 0) {
                    if (time_ranks_named(who, (size_t) ctx->height, (size_t) ctx->width, spec, bin, n_frames, row0, col0, &plan) < 0) return false;
                    if (!streams || !sizes) { set_error("%s: bad arguments", who); return false; }
                    ns.fill(n_frames, bin, [&](size_t f, uint32_t b) {
                        if (!plan.mask[b]) return 0;
                        ns.add(streams[f], sizes[f]);
                        return 1;
                    });
                    a.parsed_first = true;
                    a.ready = [&] { rank_begin(ctx, plan); return true; };
                }
                ns.ask(a);
                a.names = ns.names.data(); a.out = spec;
                a.box = ebcc_hip_region{row0, col0, spec->rows, spec->cols};
                a.decode_mark = "quantile: decode";
                return true;
            }, [&](ebcc_hip_ctx *set, const float *decoded, size_t lo, size_t k, PhaseTimer &pt) {
                rank_count(set, plan, decoded, k, ns.bn.data() + lo, pass);
                pt.mark("quantile: count");
            }, true);
            if (rc) return rc;
            rank_advance(ctx, plan, pass, spec->d_out);
        }
        std::copy(plan.count.begin(), plan.count.end(), spec->count);
        return 0;
    });
}

// ---- time-map decode: weighted sums over time per pixel (include/ebcc_hip.h: ebcc_hip_time_map; k_time_map, time_map.hip)
// Built as reduce_shard is: the frames some term names are the call the decode sees, and the fold is ordered - an output's
// additions are in frame order.  slot[f]: the place frame f has among the named ones; a batch is the frames names[lo] ..
// names[lo + k - 1] and folds the terms whose frame lies among them.
int project_shard(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, size_t row0, size_t col0,
                  const ebcc_hip_time_map *map)
{
    std::vector<const uint8_t *> st;
    std::vector<size_t> sz, names;
    std::vector<uint32_t> named, slot;
    const int rc = consume_decoded(who, ctx, false, true, [&](DecodedAsk &a) {
        if (time_map_named(who, (size_t) ctx->height, (size_t) ctx->width, map, n_frames, row0, col0, &named) < 0) return false;
        if (!streams || !sizes) { set_error("%s: bad arguments", who); return false; }
        slot.assign((size_t) named.back() + 1, 0u);
        for (const uint32_t f : named) {
            slot[f] = (uint32_t) st.size();
            st.push_back(streams[f]); sz.push_back(sizes[f]); names.push_back(f);
        }
        a.streams = st.data(); a.sizes = sz.data(); a.n = st.size(); a.names = names.data(); a.out = map;
        a.box = ebcc_hip_region{row0, col0, map->rows, map->cols};
        a.parsed_first = true;
        a.decode_mark = "project: decode";
        return true;
    }, [&](ebcc_hip_ctx *set, const float *decoded, size_t lo, size_t k, PhaseTimer &pt) {
        time_map(set, decoded, map->rows * map->cols, *map, names[lo], names[lo + k - 1] + 1, slot.data(), lo);
        pt.mark("project: fold");
    });
    if (!rc) for (size_t o = 0; o < map->n_out; o++) map->count[o] += map->start[o + 1] - map->start[o];
    return rc;
}

// ---- pair decode: co-moments and vector magnitude of two variables over time (include/ebcc_hip.h: ebcc_hip_pair_stats; k_pair_fold, pair_stats.hip)
// Built as reduce_shard is, with two streams to a step: the decode sees the named steps' streams interleaved - item 2i is the x
// and item 2i + 1 the y of the i-th named step - and asks for batches of an even number of frames (DecodedAsk::granule), so the
// two frames of a step lie in the same batch, whose fold gets the audit buffer as both bases.  The fold is ordered: a bin's
// additions are in step order.  The pre-parse is the call's own: its message names the step and says x or y.
int pair_shard(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *x_streams, const size_t *x_sizes, const uint8_t *const *y_streams,
               const size_t *y_sizes, size_t n_steps, const uint32_t *bin, size_t row0, size_t col0, const ebcc_hip_pair_stats *stats)
{
    NamedSteps ns;
    const int rc = consume_decoded(who, ctx, false, true, [&](DecodedAsk &a) {
        if (pair_stats_named(who, (size_t) ctx->height, (size_t) ctx->width, stats, bin, n_steps, row0, col0) < 0) return false;
        if (!x_streams || !x_sizes || !y_streams || !y_sizes) { set_error("%s: bad arguments", who); return false; }
        if (ctx->max_frames < 2) { set_error("%s: a context of capacity 1 cannot hold the two frames of a step", who); return false; }
        const bool parsed = ns.fill(n_steps, bin, [&](size_t t, uint32_t) {
            ParsedFrame pf;
            if (!x_streams[t] || !parse_frame(x_streams[t], x_sizes[t], pf)) { set_error("%s: step %zu: x is not a frame stream", who, t); return -1; }
            if (!y_streams[t] || !parse_frame(y_streams[t], y_sizes[t], pf)) { set_error("%s: step %zu: y is not a frame stream", who, t); return -1; }
            ns.add(x_streams[t], x_sizes[t]);
            ns.add(y_streams[t], y_sizes[t]);
            return 1;
        });
        if (!parsed) return false;
        ns.ask(a);
        a.out = stats;
        a.box = ebcc_hip_region{row0, col0, stats->rows, stats->cols};
        a.granule = 2;
        a.decode_mark = "pair: decode";
        return true;
    }, [&](ebcc_hip_ctx *set, const float *decoded, size_t lo, size_t k, PhaseTimer &pt) {
        pair_fold(set, decoded, decoded, true, k / 2, stats->rows * stats->cols, ns.bn.data() + lo / 2, *stats);
        pt.mark("pair: fold");
    });
    if (!rc) ns.add_counts(stats->count);
    return rc;
}

// ---- spell decode: run lengths and event timing over time (include/ebcc_hip.h: ebcc_hip_spell_stats; k_spell_fold, spell_stats.hip)
// Built as reduce_shard is: the named steps are the call the decode sees, with their labels (a step's index in the caller's
// list where there is no `when`) and flags; the fold is ordered: a bin's steps are in step order, and the run a batch ends with
// is in d_run when the next batch begins.
int spell_shard(const char *who, ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin,
                const uint32_t *when, const uint8_t *fresh, size_t row0, size_t col0, const ebcc_hip_spell_stats *stats)
{
    NamedSteps ns;
    std::vector<uint32_t> wh;
    std::vector<uint8_t> fr;
    const int rc = consume_decoded(who, ctx, false, true, [&](DecodedAsk &a) {
        if (spell_stats_named(who, (size_t) ctx->height, (size_t) ctx->width, stats, bin, when, n_frames, row0, col0) < 0) return false;
        if (!streams || !sizes) { set_error("%s: bad arguments", who); return false; }
        ns.fill(n_frames, bin, [&](size_t f, uint32_t) {
            ns.add(streams[f], sizes[f]);
            wh.push_back(when ? when[f] : (uint32_t) f); fr.push_back(fresh && fresh[f] ? 1 : 0);
            return 1;
        });
        ns.ask(a);
        a.names = ns.names.data(); a.out = stats;
        a.box = ebcc_hip_region{row0, col0, stats->rows, stats->cols};
        a.parsed_first = true;
        a.decode_mark = "spell: decode";
        return true;
    }, [&](ebcc_hip_ctx *set, const float *decoded, size_t lo, size_t k, PhaseTimer &pt) {
        spell_fold(set, decoded, k, stats->rows * stats->cols, ns.bn.data() + lo, wh.data() + lo, fr.data() + lo, *stats);
        pt.mark("spell: fold");
    });
    if (!rc) ns.add_counts(stats->count);
    return rc;
}

// ---- EBCK chunk container (the reference's src/ebcc_codec.c:920-1052, :1322-1449) --------------------------------------------------
// The container as ebcc_decode_chunking checks it: the header, then the chain of `u64 nbytes | stream` entries - of a chunk only
// the length field is read.  parse: "" or what is wrong with it (the reference's messages).
struct Container {
    size_t dims[3], cd[3], cnt[3], csize = 0, nchunks = 0, total = 0;
    std::vector<const uint8_t *> ptrs;
    std::vector<size_t> lens;
    std::string parse(const uint8_t *data, size_t data_size)
    {
        char text[160];
        if (!data || data_size < sizeof(ChunkHeader) || memcmp(data, EBCC_CHUNKING_HEADER_MAGIC, 4) != 0) return "not an EBCK chunk container";
        ChunkHeader hd;
        memcpy(&hd, data, sizeof hd);
        if (hd.version != EBCC_CHUNKING_HEADER_VERSION) { snprintf(text, sizeof text, "Unsupported EBCC chunking header version: %u", hd.version); return text; }
        if (hd.ndims != NDIMS) { snprintf(text, sizeof text, "Unsupported EBCC chunking dimensionality: %u", hd.ndims); return text; }
        for (int i = 0; i < 3; i++) { dims[i] = hd.dims[i]; cd[i] = hd.chunk_dims[i]; }
        if (!dims_are_valid(cd)) return "Invalid chunked EBCC data: bad chunk dimensions";
        for (int i = 0; i < 3; i++) {
            if (!dims[i] || !cd[i]) return "Invalid chunked EBCC data: dims and chunk_dims must be non-zero";
            cnt[i] = cdiv(dims[i], cd[i]);
        }
        csize = cd[0] * cd[1] * cd[2]; nchunks = cnt[0] * cnt[1] * cnt[2]; total = dims[0] * dims[1] * dims[2];
        if (hd.chunk_size != csize || hd.num_chunks != nchunks) return "Invalid chunked EBCC data: inconsistent chunk metadata";
        if (cd[0] != 1 && !tile_height_supported(cd[1])) {
            snprintf(text, sizeof text, "chunks holding %lu frames of %lu rows are not supported", cd[0], cd[1]);
            return text;
        }
        ptrs.resize(nchunks); lens.resize(nchunks);
        const uint8_t *p = data + sizeof hd, *end = data + data_size;
        for (size_t c = 0; c < nchunks; c++) {
            uint64_t nb;
            if ((size_t) (end - p) < 8) return "Invalid chunked EBCC data: missing chunk size";
            memcpy(&nb, p, 8); p += 8;
            if (nb > (size_t) (end - p)) return "Invalid chunked EBCC data: truncated chunk payload";
            ptrs[c] = p; lens[c] = nb; p += nb;
        }
        if (p != end) return "Invalid chunked EBCC data: trailing payload bytes";
        return "";
    }
};

// A slab of a container of one-frame chunks as the placed boxes of the chunks it meets (ebcc_hip_slab_plan), against a compact
// [nt][rows][cols] output; false: refused, message set.  (H, W: the geometry of the engine that is to decode it, 0: any)
bool slab_boxes(const char *who, Container &box, const uint8_t *data, size_t size, const ebcc_hip_slab *slab, size_t H, size_t W,
                std::vector<ebcc_hip_placed_box> &boxes)
{
    const std::string bad = box.parse(data, size);
    if (!bad.empty()) { set_error("%s: %s", who, bad.c_str()); return false; }
    if (box.cd[0] != 1) { set_error("%s: chunks of several frames (%zu) are not supported", who, box.cd[0]); return false; }
    if (H && (box.cd[1] != H || box.cd[2] != W)) {
        set_error("%s: the context's frames are %zu x %zu, the container's chunks %zu x %zu", who, H, W, box.cd[1], box.cd[2]);
        return false;
    }
    const long n = slab ? ebcc_hip_slab_plan(box.dims, box.cd, slab, nullptr, 0) : -1;
    if (n < 0) {
        if (slab) set_error("%s: the slab [%zu, +%zu) x [%zu, +%zu) x [%zu, +%zu) is empty or not inside the (%zu, %zu, %zu) array", who, slab->t0, slab->nt,
                            slab->row0, slab->rows, slab->col0, slab->cols, box.dims[0], box.dims[1], box.dims[2]);
        else set_error("%s: bad arguments", who);
        return false;
    }
    boxes.resize((size_t) n);
    ebcc_hip_slab_plan(box.dims, box.cd, slab, boxes.data(), boxes.size());
    return true;
}
int container_slab(const char *who, ebcc_hip_ctx *ctx, const uint8_t *data, size_t size, const ebcc_hip_slab *slab, float *out, bool host)
{
    if (!ctx || !out) { set_error("%s: bad arguments", who); return 1; }
    Container box;
    std::vector<ebcc_hip_placed_box> boxes;
    if (!slab_boxes(who, box, data, size, slab, (size_t) ctx->height, (size_t) ctx->width, boxes)) return 1;
    const DecodeRegion region = DecodeRegion::placed_list(boxes.data(), boxes.size(), slab->nt * slab->rows * slab->cols);
    return host ? decode_host(who, ctx, box.ptrs.data(), box.lens.data(), box.nchunks, out, region, false)
                : decode_resident(who, ctx, box.ptrs.data(), box.lens.data(), box.nchunks, out, region, false);
}

// The container of the chunk streams outs[c] / sizes[c] (:975-992, :1028-1046): header, then `u64 nbytes | stream` per chunk.
// malloc'd, NULL without memory (logged); the streams stay the caller's.
uint8_t *assemble_container(const size_t dims[3], const size_t cd[3], size_t nchunks, size_t csize, uint8_t *const *outs, const size_t *sizes, size_t *out_len)
{
    size_t len = sizeof(ChunkHeader);
    for (size_t c = 0; c < nchunks; c++) len += 8 + sizes[c];
    uint8_t *o = (uint8_t *) malloc(len), *p = o;
    if (!o) { log_fatal("out of memory"); return nullptr; }
    ChunkHeader hd;
    memset(&hd, 0, sizeof hd);
    memcpy(hd.magic, EBCC_CHUNKING_HEADER_MAGIC, 4);
    hd.version = EBCC_CHUNKING_HEADER_VERSION; hd.ndims = NDIMS;
    for (int i = 0; i < 3; i++) { hd.dims[i] = dims[i]; hd.chunk_dims[i] = cd[i]; }
    hd.num_chunks = nchunks; hd.chunk_size = csize;
    memcpy(p, &hd, sizeof hd); p += sizeof hd;
    for (size_t c = 0; c < nchunks; c++) {
        uint64_t nb = sizes[c];
        memcpy(p, &nb, 8); p += 8;
        memcpy(p, outs[c], sizes[c]); p += sizes[c];
    }
    *out_len = len;
    return o;
}

// ---- container encode from the device ---------------------------------------------------------------
// What ebcc_encode_chunking (compat: ebcc_encode_chunking_compat, :1059-1076) makes of config->dims / chunk_dims: the chunk
// dims, counts and sizes, or what it refuses - and, which the host scan leaves out, a product of the dims that overflows
// (:953-964, :1079-1083).  "" or the message.
struct ContainerPlan {
    ChunkBox box;
    size_t csize = 0, nchunks = 0, total = 0, padded = 0;
    std::string make(const codec_config_t *cfg, bool compat)
    {
        char text[200];
        const size_t *dims = cfg->dims;
        size_t *cd = box.cd;
        bool all_zero = true;
        for (int i = 0; i < 3; i++) { box.dims[i] = dims[i]; cd[i] = cfg->chunk_dims[i]; if (cd[i]) all_zero = false; }
        if (all_zero) {
            cd[0] = compat ? 1 : dims[0];
            for (int i = 1; i < 3; i++) cd[i] = compat && dims[i] > EBCC_MAX_INTERNAL_IMAGE_DIM ? 1024 : dims[i];
        }
        if (!dims_are_valid(cd)) {
            snprintf(text, sizeof text, "Invalid chunking dimensions: product(chunk_dims[0..1]) and chunk_dims[2] must be between %d and %d",
                     EBCC_MIN_INTERNAL_IMAGE_DIM, EBCC_MAX_INTERNAL_IMAGE_DIM);
            return text;
        }
        for (int i = 0; i < 3; i++) {
            if (dims[i] == 0 || cd[i] == 0) return "Invalid chunking dimensions: dims and chunk_dims must be non-zero";
            box.cnt[i] = cdiv(dims[i], cd[i]);
        }
        if (cd[0] != 1 && !tile_height_supported(cd[1])) {
            snprintf(text, sizeof text, "chunks holding %zu frames of %zu rows are not supported; use chunk_dims[0] = 1", cd[0], cd[1]);
            return text;
        }
        auto product = [](const size_t v[3], size_t *out) { return !__builtin_mul_overflow(v[0], v[1], out) && !__builtin_mul_overflow(*out, v[2], out); };
        size_t bytes;
        if (!product(cd, &csize) || !product(box.cnt, &nchunks) || !product(dims, &total) || __builtin_mul_overflow(total, sizeof(float), &bytes))
            return "Invalid chunking dimensions: size overflow";
        if (__builtin_mul_overflow(csize, nchunks, &padded) || __builtin_mul_overflow(padded, sizeof(float), &bytes))
            return "Invalid chunking dimensions: padded size overflow";
        return "";
    }
    void warn_padding() const                                   // :965-969
    {
        if (padded > total && padded - total > total / 10)
            log_warn("Chunk padding adds %lu values over %lu real values (%.2f%%)", padded - total, total, ((double) (padded - total) / (double) total) * 100.0);
    }
};

// The checks of the two encode entry points, in their order: the plan, one-frame chunks, the context's geometry, the range of
// chunks (count 0: all of them).  0, or 1 with the message set.
int array_plan(const char *who, ebcc_hip_ctx *ctx, const codec_config_t *cfg, bool compat, bool defaults, size_t first, size_t count, ContainerPlan &plan)
{
    if (!defaults && !cfg->chunk_dims[0] && !cfg->chunk_dims[1] && !cfg->chunk_dims[2]) { set_error("%s: config->chunk_dims must be set", who); return 1; }
    const std::string bad = plan.make(cfg, compat);
    if (!bad.empty()) { set_error("%s: %s", who, bad.c_str()); return 1; }
    const size_t *cd = plan.box.cd;
    if (cd[0] != 1) { set_error("%s: chunks of %zu frames (one-frame chunks only)", who, cd[0]); return 1; }
    if (cd[1] != (size_t) ctx->height || cd[2] != (size_t) ctx->width) {
        set_error("%s: the context's frames are %d x %d, the chunks %zu x %zu", who, ctx->height, ctx->width, cd[1], cd[2]);
        return 1;
    }
    if (first > plan.nchunks || count > plan.nchunks - first) {
        set_error("%s: chunks [%zu, +%zu) of %zu", who, first, count, plan.nchunks);
        return 1;
    }
    return 0;
}

// The streams of chunks [first, first + count) of a planned array on the device: batches of the context's capacity on the
// alternating sets.  A batch's padded chunks are gathered into its engine set's staging buffer, on that set's stream, and the
// stage waits for them: the slices read them on streams of their own.  Chunks that are whole frames are coded where they lie.
int encode_array_chunks(const char *who, ebcc_hip_ctx *ctx, const float *d_array, const codec_config_t *cfg, const ContainerPlan &plan,
                        size_t first, size_t count, uint8_t **outs, size_t *sizes)
{
    const ChunkBox &box = plan.box;
    codec_config_t cc = *cfg;
    for (int i = 0; i < 3; i++) { cc.dims[i] = box.cd[i]; cc.chunk_dims[i] = 0; }
    const size_t csize = plan.csize, cap = std::min(count, ctx->max_frames);
    PhaseTimer pt[2];
    const std::vector<FrameConfig> fc(count, FrameConfig(cc));
    return encode_call(who, ctx, d_array, count, &cc, outs, sizes, [&] {
        return encode_batches_alternating(ctx, count, fc.data(), outs, sizes, [&](ebcc_hip_ctx *set, size_t lo, size_t cnt) {
            if (box.slabs()) return d_array + (first + lo) * csize;
            float *d = io_buffer(set, cap * csize * sizeof(float));
            launch_gather_chunks(d_array, box.dims[1], box.dims[2], box.cd[1], box.cd[2], first + lo, cnt, d, set->stream);
            wait_stream(set->stream);
            pt[set != ctx].mark("array chunks: gather");
            return (const float *) d;
        });
    });
}

// ---- what the entry points of the decodes over time share
// <x>_init: every array of `fills` that is there set to n elements of its start value - zero bytes, or a 32-bit word (elements of
// 4 bytes) - on the context's stream, which is waited for; then count[0 .. n_count) = 0.
struct StartValue { void *d; size_t elem; uint32_t word; };
constexpr uint32_t kPlusInf = 0x7F800000u, kMinusInf = 0xFF800000u;
int start_values(ebcc_hip_ctx *ctx, std::initializer_list<StartValue> fills, size_t n, uint64_t *count, size_t n_count)
{
    return on_device(ctx->device, 1, [&] {
        for (const StartValue &f : fills) {
            if (!f.d) continue;
            if (f.word) EBCC_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t) f.d, (int) f.word, n, ctx->stream));
            else EBCC_HIP_CHECK(hipMemsetAsync(f.d, 0, n * f.elem, ctx->stream));
        }
        wait_stream(ctx->stream);
        std::fill_n(count, n_count, (uint64_t) 0);
        return 0;
    });
}
// <x>_fold / <x>_items: the refusal of the context and of the item arrays, check() (< 0: refused, the message set), then body()
// on the context's device.
template <class Check, class Body>
int items_call(const char *who, ebcc_hip_ctx *ctx, std::initializer_list<const float *> items, size_t n_items, Check check, Body body)
{
    bool bad = !ctx || n_items >= 0xFFFFFFFFu;
    for (const float *p : items) bad = bad || !p || ((uintptr_t) p & 3);
    if (bad) { set_error("%s: bad arguments", who); return 1; }
    if (check() < 0) return 1;
    return on_device(ctx->device, 1, [&] { body(); return 0; });
}
// count[bin] += 1 for every item that `bin` names
void count_named(size_t n, const uint32_t *bin, uint64_t *count)
{
    for (size_t k = 0; k < n; k++)
        if (!bin || bin[k] != EBCC_HIP_NO_BIN) count[bin ? bin[k] : 0u]++;
}

}  // namespace

namespace ebcc {

int cached_encode_host_frames(const float *h_frames, size_t n, int H, int W, const codec_config_t *cfg, uint8_t **outs, size_t *sizes)
{
    return encode_on_device(resolve_device(), h_frames, n, H, W, cfg, outs, sizes);
}

int cached_decode_host_frames(const uint8_t *const *streams, const size_t *sizes, size_t n, int H, int W, float *h_out)
{
    const int device = resolve_device();
    return on_codec(device, 1, [&] {
        ebcc_hip_ctx *ctx = nullptr, *rc = nullptr;
        if (!chunk_engines(device, H, W, std::min(n, batch_capacity((size_t) H * W)), 1, &ctx, &rc)) return 1;
        return decode_to_host(ctx, nullptr, 1, ctx->max_frames, streams, sizes, n, h_out, nullptr);
    });
}

}  // namespace ebcc

extern "C" {

void free_buffer(void *p) { if (p) free(p); }

void log_set_level_from_env(void)
{
    g_log_level = 3;
    if (const char *e = getenv("EBCC_LOG_LEVEL")) {
        char *end;
        long v = strtol(e, &end, 10);
        if (*end != '\0') log_warn("Ignore log level: %s, should be in [0, 5]", e);
        else g_log_level = (int) v;
    }
}

void print_config(codec_config_t *c)
{
    static const char *names[] = {"NONE", "MAX_ERROR", "RELATIVE_ERROR"};
    log_info("dimensions:\t(%lu, %lu, %lu)", c->dims[0], c->dims[1], c->dims[2]);
    log_info("chunk dimensions:\t(%lu, %lu, %lu)", c->chunk_dims[0], c->chunk_dims[1], c->chunk_dims[2]);
    log_info("base_cr:\t%f", c->base_cr);
    unsigned t = (unsigned) c->residual_compression_type;
    log_info("residual type:\t%s", t < 3 ? names[t] : "?");
    if (t == MAX_ERROR) log_info("max error:\t%f", c->error);
    if (t == RELATIVE_ERROR) log_info("relative error:\t%f", c->error);
}

int ebcc_hip_host_threads(int slices) { return (int) entropy_threads((unsigned) std::max(1, slices)); }
int ebcc_hip_default_encode_slices(void) { return (int) default_encode_slices(); }
int ebcc_hip_encode_slices_for(size_t n_frames) { return (int) slice_count(n_frames, "EBCC_HIP_SLICES", default_encode_slices()); }

// out[0..6] = usable CPUs (affinity mask cut to the cgroup quota), CPU quota (0: none), zstd core-seconds, seconds the
// slices waited for the zstd workers, bytes compressed, entropy batches, prefix bytes whose compression was proved
// unnecessary - since the last call with reset != 0
// arithmetic identities the kernels rely on, checked on the host (0 = all hold): the division-free s / 65535.0f of the fused
// inverse level for every s in [0, 65535]; v / 255.0f and x / kXi of the residual synthesis (all significands)
int ebcc_hip_selfcheck(void) { return j2k_selfcheck_div65535() + residual_selfcheck_divisions(); }
void ebcc_hip_plan_decode_lanes(const int *table, int n_code_blocks, int out[4]) { plan_decode_lanes(table, std::max(0, n_code_blocks), out); }

// the lower bound of zstd_size_lower_bound (0: not applicable - longer than 4 MB, or a libzstd that may split blocks)
size_t ebcc_hip_zstd_floor(const uint8_t *src, size_t n) { return zstd_floor_usable() ? zstd_size_lower_bound(src, n) : 0; }

void ebcc_hip_host_stats(double *out, int reset)
{
    HostStats &h = host_stats();
    if (out) {
        out[0] = (double) usable_cpus(); out[1] = cgroup_cpu_quota();
        out[2] = h.zstd_core_us.load() / 1e6; out[3] = h.zstd_wait_us.load() / 1e6;
        out[4] = (double) h.zstd_bytes.load(); out[5] = (double) h.batches.load(); out[6] = (double) h.skipped_bytes.load();
    }
    if (reset) h.reset();
}

// A pageable host array <-> device memory at PCIe speed: through the engine's two pinned bounce buffers with several host
// threads copying (copy_pageable) instead of hipMemcpy's single staging thread (~10 GB/s, and a fresh destination's page
// faults on top) - what ebcc_decode_chunking does for its own output, for callers of the frames API that keep their
// frames in host memory (ebcc_amd/h5_batch.py).  Return 0 = ok.
int ebcc_hip_upload(ebcc_hip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    if (!ctx || !d_dst || !h_src) { set_error("ebcc_hip_upload: null argument"); return 1; }
    return on_device(ctx->device, 1, [&] {
        copy_pageable(ctx, const_cast<void *>(h_src), d_dst, bytes, false);
        return 0;
    });
}
int ebcc_hip_download(ebcc_hip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    if (!ctx || !h_dst || !d_src) { set_error("ebcc_hip_download: null argument"); return 1; }
    return on_device(ctx->device, 1, [&] {
        huge_pages(h_dst, bytes);                                       // (a fresh array: fewer faults)
        copy_pageable(ctx, h_dst, const_cast<void *>(d_src), bytes, true);
        return 0;
    });
}

// The pages of a host array that is about to receive a download, mapped by several threads (huge pages where granted);
// returns when they are.  Meant to run on a caller's thread beside ebcc_hip_decode_frames.  Return 0 = ok.
int ebcc_hip_prefault(void *h_dst, size_t bytes)
{
    EBCC_API_TRY
    if (!h_dst) { set_error("ebcc_hip_prefault: null argument"); return 1; }
    Prefault pf(h_dst, bytes);
    pf.join();
    return 0;
    EBCC_API_CATCH(1)
}

// Frames in pageable host memory <-> streams through a caller's context, for callers that keep the chunks themselves
// (ebcc_amd/h5_batch.py: HDF5 direct chunk writes / reads): what ebcc_encode_chunking / ebcc_decode_chunking do between the
// array and the EBCK container - uploads / downloads through the pinned bounce buffers, batches of the context's capacity
// on the two alternating engine sets, the output's pages mapped while the GPU decodes.  Any number of frames.  0 = ok;
// on error every stream made so far has been freed.
int ebcc_hip_encode_host_frames(ebcc_hip_ctx *ctx, const float *h_frames, size_t n_frames, const codec_config_t *config,
                                uint8_t **out_streams, size_t *out_sizes)
{
    const int rc = encode_call("ebcc_hip_encode_host_frames", ctx, h_frames, n_frames, config, out_streams, out_sizes, [&] {
        return encode_from_host(ctx, nullptr, 1, ctx->max_frames, h_frames, n_frames, config, out_streams, out_sizes);
    });
    if (rc == 2) set_error("ebcc_hip_encode_host_frames: NaN or Inf in the data");
    return rc;
}
int ebcc_hip_decode_host_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, float *h_frames_out)
{
    return decode_host("ebcc_hip_decode_host_frames", ctx, streams, sizes, n_frames, h_frames_out, DecodeRegion{});
}

// Window decode: the box [row0, row0 + rows) x [col0, col0 + cols) of every frame, bit for bit the crop of what the entry
// point without a window gives, from the code-blocks the box depends on (J2kWindow, j2k.hpp); output [n][rows][cols].
int ebcc_hip_decode_frames_window(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, size_t row0, size_t col0,
                                  size_t rows, size_t cols, float *d_out)
{
    return decode_resident("ebcc_hip_decode_frames_window", ctx, streams, sizes, n_frames, d_out, DecodeRegion::window(row0, col0, rows, cols), true);
}
int ebcc_hip_decode_shard_window(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, size_t row0, size_t col0,
                                 size_t rows, size_t cols, float *d_out)
{
    return decode_resident("ebcc_hip_decode_shard_window", ctx, streams, sizes, n_frames, d_out, DecodeRegion::window(row0, col0, rows, cols), false);
}
int ebcc_hip_decode_host_frames_window(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, size_t row0, size_t col0,
                                       size_t rows, size_t cols, float *h_out)
{
    return decode_host("ebcc_hip_decode_host_frames_window", ctx, streams, sizes, n_frames, h_out, DecodeRegion::window(row0, col0, rows, cols));
}

// Box-list decode: boxes of rows x cols, each from the frame it names, bit for bit the crops of what the entry points without
// boxes give; output [n_boxes][rows][cols] (decode_boxes).
int ebcc_hip_decode_frames_boxes(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_box *boxes,
                                 size_t n_boxes, size_t rows, size_t cols, float *d_out)
{
    EBCC_API_TRY
    return decode_boxes("ebcc_hip_decode_frames_boxes", ctx, streams, sizes, n_frames, boxes, n_boxes, rows, cols, d_out, false, true);
    EBCC_API_CATCH(1)
}
int ebcc_hip_decode_shard_boxes(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_box *boxes,
                                size_t n_boxes, size_t rows, size_t cols, float *d_out)
{
    EBCC_API_TRY
    return decode_boxes("ebcc_hip_decode_shard_boxes", ctx, streams, sizes, n_frames, boxes, n_boxes, rows, cols, d_out, false, false);
    EBCC_API_CATCH(1)
}
int ebcc_hip_decode_host_frames_boxes(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_box *boxes,
                                      size_t n_boxes, size_t rows, size_t cols, float *h_out)
{
    EBCC_API_TRY
    return decode_boxes("ebcc_hip_decode_host_frames_boxes", ctx, streams, sizes, n_frames, boxes, n_boxes, rows, cols, h_out, true, false);
    EBCC_API_CATCH(1)
}

// Placed boxes: boxes of their own sizes, each to its own rectangle of the output (include/ebcc_hip.h).
int ebcc_hip_decode_frames_placed(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_placed_box *boxes,
                                  size_t n_boxes, float *d_out, size_t out_floats)
{
    EBCC_API_TRY
    return decode_resident("ebcc_hip_decode_frames_placed", ctx, streams, sizes, n_frames, d_out, DecodeRegion::placed_list(boxes, n_boxes, out_floats), true);
    EBCC_API_CATCH(1)
}
int ebcc_hip_decode_shard_placed(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_placed_box *boxes,
                                 size_t n_boxes, float *d_out, size_t out_floats)
{
    EBCC_API_TRY
    return decode_resident("ebcc_hip_decode_shard_placed", ctx, streams, sizes, n_frames, d_out, DecodeRegion::placed_list(boxes, n_boxes, out_floats), false);
    EBCC_API_CATCH(1)
}
int ebcc_hip_decode_host_frames_placed(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_placed_box *boxes,
                                       size_t n_boxes, float *h_out, size_t out_floats)
{
    EBCC_API_TRY
    return decode_host("ebcc_hip_decode_host_frames_placed", ctx, streams, sizes, n_frames, h_out, DecodeRegion::placed_list(boxes, n_boxes, out_floats), false);
    EBCC_API_CATCH(1)
}

// A slab of an array in chunks as placed boxes (include/ebcc_hip.h; host only, no device work).
long ebcc_hip_slab_plan(const size_t dims[3], const size_t chunk_dims[3], const ebcc_hip_slab *slab, ebcc_hip_placed_box *boxes, size_t max_boxes)
{
    EBCC_API_TRY
    if (!dims || !chunk_dims || !slab) { set_error("ebcc_hip_slab_plan: bad arguments"); return -1; }
    const size_t *cd = chunk_dims;
    if (!dims[0] || !dims[1] || !dims[2]) { set_error("ebcc_hip_slab_plan: zero dims"); return -1; }
    if (cd[0] != 1) { set_error("ebcc_hip_slab_plan: chunks of %zu frames (one-frame chunks only)", cd[0]); return -1; }
    if (!dims_are_valid(cd)) { set_error("ebcc_hip_slab_plan: chunks of %zu x %zu are not between %d and %d", cd[1], cd[2], EBCC_MIN_INTERNAL_IMAGE_DIM, EBCC_MAX_INTERNAL_IMAGE_DIM); return -1; }
    const size_t org[3] = {slab->t0, slab->row0, slab->col0}, ext[3] = {slab->nt, slab->rows, slab->cols};
    for (int i = 0; i < 3; i++)
        if (ext[i] < 1 || org[i] >= dims[i] || ext[i] > dims[i] - org[i]) {       // (no sums: they may overflow)
            set_error("ebcc_hip_slab_plan: the slab is empty or not inside the (%zu, %zu, %zu) array", dims[0], dims[1], dims[2]);
            return -1;
        }
    const size_t cnt1 = cdiv(dims[1], cd[1]), cnt2 = cdiv(dims[2], cd[2]);
    const size_t cy0 = org[1] / cd[1], cy1 = (org[1] + ext[1] - 1) / cd[1], cx0 = org[2] / cd[2], cx1 = (org[2] + ext[2] - 1) / cd[2];
    const size_t count = ext[0] * (cy1 - cy0 + 1) * (cx1 - cx0 + 1);
    if (count > (size_t) LONG_MAX) { set_error("ebcc_hip_slab_plan: too many chunks"); return -1; }
    if (!boxes) return (long) count;
    if (max_boxes < count) { set_error("ebcc_hip_slab_plan: room for %zu of %zu boxes", max_boxes, count); return -1; }
    ebcc_hip_placed_box *b = boxes;
    for (size_t t = org[0]; t < org[0] + ext[0]; t++)
        for (size_t cy = cy0; cy <= cy1; cy++)
            for (size_t cx = cx0; cx <= cx1; cx++, b++) {
                // the slab cut with the chunk (the slab lies inside the array: so does the cut, in the chunk's real part)
                const size_t r0 = std::max(org[1], cy * cd[1]), r1 = std::min(org[1] + ext[1], (cy + 1) * cd[1]);
                const size_t c0 = std::max(org[2], cx * cd[2]), c1 = std::min(org[2] + ext[2], (cx + 1) * cd[2]);
                *b = ebcc_hip_placed_box{(t * cnt1 + cy) * cnt2 + cx, r0 - cy * cd[1], c0 - cx * cd[2], r1 - r0, c1 - c0,
                                         ((t - org[0]) * ext[1] + (r0 - org[1])) * ext[2] + (c0 - org[2]), ext[2]};
            }
    return (long) count;
    EBCC_API_CATCH(-1)
}

int ebcc_hip_container_info(const uint8_t *data, size_t size, size_t dims[3], size_t chunk_dims[3])
{
    EBCC_API_TRY
    Container box;
    const std::string bad = box.parse(data, size);
    if (!bad.empty()) { set_error("ebcc_hip_container_info: %s", bad.c_str()); return 1; }
    for (int i = 0; i < 3; i++) { if (dims) dims[i] = box.dims[i]; if (chunk_dims) chunk_dims[i] = box.cd[i]; }
    return 0;
    EBCC_API_CATCH(1)
}

int ebcc_hip_decode_container_slab(ebcc_hip_ctx *ctx, const uint8_t *data, size_t size, const ebcc_hip_slab *slab, float *d_out)
{
    EBCC_API_TRY
    return container_slab("ebcc_hip_decode_container_slab", ctx, data, size, slab, d_out, false);
    EBCC_API_CATCH(1)
}
int ebcc_hip_decode_container_slab_host(ebcc_hip_ctx *ctx, const uint8_t *data, size_t size, const ebcc_hip_slab *slab, float *h_out)
{
    EBCC_API_TRY
    return container_slab("ebcc_hip_decode_container_slab_host", ctx, data, size, slab, h_out, true);
    EBCC_API_CATCH(1)
}

// ---- container encode from the device (include/ebcc_hip.h) ------------------------------------------
int ebcc_hip_container_plan(const codec_config_t *config, int compat, size_t chunk_dims[3], size_t *n_chunks)
{
    EBCC_API_TRY
    if (!config) { set_error("ebcc_hip_container_plan: bad arguments"); return 1; }
    ContainerPlan plan;
    const std::string bad = plan.make(config, compat != 0);
    if (!bad.empty()) { set_error("ebcc_hip_container_plan: %s", bad.c_str()); return 1; }
    for (int i = 0; i < 3; i++) if (chunk_dims) chunk_dims[i] = plan.box.cd[i];
    if (n_chunks) *n_chunks = plan.nchunks;
    return 0;
    EBCC_API_CATCH(1)
}

int ebcc_hip_array_range(ebcc_hip_ctx *ctx, const float *d_data, size_t n, float minmax[2])
{
    if (!ctx || !d_data || !minmax || n < 1) { set_error("ebcc_hip_array_range: bad arguments"); return 1; }
    return on_device(ctx->device, 1, [&] {
        const int rc = array_range(ctx, d_data, n, minmax);
        if (rc == 2) set_error("ebcc_hip_array_range: NaN or Inf found in the data");
        return rc;
    });
}

int ebcc_hip_gather_chunks(ebcc_hip_ctx *ctx, const float *d_array, const size_t dims[3], const size_t chunk_dims[3], size_t first, size_t count,
                           float *d_out)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_gather_chunks";
    if (!ctx || !d_array || !dims || !chunk_dims || !d_out || count < 1) { set_error("%s: bad arguments", who); return 1; }
    codec_config_t cfg{};
    for (int i = 0; i < 3; i++) { cfg.dims[i] = dims[i]; cfg.chunk_dims[i] = chunk_dims[i]; }
    ContainerPlan plan;
    if (!dims[0] || !dims[1] || !dims[2]) { set_error("%s: zero dims", who); return 1; }
    const std::string bad = plan.make(&cfg, false);
    if (!bad.empty()) { set_error("%s: %s", who, bad.c_str()); return 1; }
    if (chunk_dims[0] != 1) { set_error("%s: chunks of %zu frames (one-frame chunks only)", who, chunk_dims[0]); return 1; }
    if (first > plan.nchunks || count > plan.nchunks - first) { set_error("%s: chunks [%zu, +%zu) of %zu", who, first, count, plan.nchunks); return 1; }
    return on_device(ctx->device, 1, [&] {
        launch_gather_chunks(d_array, dims[1], dims[2], chunk_dims[1], chunk_dims[2], first, count, d_out, ctx->stream);
        wait_stream(ctx->stream);
        return 0;
    });
    EBCC_API_CATCH(1)
}

int ebcc_hip_encode_array_chunks(ebcc_hip_ctx *ctx, const float *d_array, const codec_config_t *config, size_t first, size_t count,
                                 uint8_t **out_streams, size_t *out_sizes)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_encode_array_chunks";
    if (!ctx || !d_array || !config || !out_streams || !out_sizes || count < 1) { set_error("%s: bad arguments", who); return 1; }
    log_set_level_from_env();
    ContainerPlan plan;
    if (array_plan(who, ctx, config, false, false, first, count, plan)) return 1;
    plan.warn_padding();
    return encode_array_chunks(who, ctx, d_array, config, plan, first, count, out_streams, out_sizes);
    EBCC_API_CATCH(1)
}

int ebcc_hip_encode_container(ebcc_hip_ctx *ctx, const float *d_array, const codec_config_t *config, int compat, uint8_t **out, size_t *out_size)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_encode_container";
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (!ctx || !d_array || !config || !out || !out_size) { set_error("%s: bad arguments", who); return 1; }
    log_set_level_from_env();
    ContainerPlan plan;
    if (array_plan(who, ctx, config, compat != 0, true, 0, 0, plan)) return 1;
    codec_config_t c = *config;
    if (compat && c.residual_compression_type == RELATIVE_ERROR) {                                 // :1078-1087
        float mm[2];
        const int rc = on_device(ctx->device, 1, [&] { return array_range(ctx, d_array, plan.total, mm); });
        if (rc == 2) { log_fatal("NaN or Inf found in data"); set_error("%s: NaN or Inf found in the data", who); }
        if (rc) return rc;
        c.error *= mm[1] - mm[0];
        c.residual_compression_type = MAX_ERROR;
    }
    plan.warn_padding();
    std::vector<uint8_t *> outs(plan.nchunks, nullptr);
    std::vector<size_t> sizes(plan.nchunks, 0);
    const int rc = encode_array_chunks(who, ctx, d_array, &c, plan, 0, plan.nchunks, outs.data(), sizes.data());
    if (rc) return rc;
    size_t len = 0;
    uint8_t *o = assemble_container(plan.box.dims, plan.box.cd, plan.nchunks, plan.csize, outs.data(), sizes.data(), &len);
    for (auto q : outs) free(q);
    if (!o) { set_error("%s: out of memory", who); return 1; }
    *out = o; *out_size = len;
    return 0;
    EBCC_API_CATCH(1)
}

// The engines the reference-compatible entry points keep between calls (one per device and frame geometry, with their slice
// engines and second set: tens of GB of device memory for 256 frames of 721 x 1440) are destroyed; the next call makes them
// again.  Contexts made with ebcc_hip_create are the caller's and are not touched.
void ebcc_hip_release_engines(void)
{
    EBCC_API_TRY
    std::vector<int> devices;
    {
        std::lock_guard<std::mutex> lock(g_map_mutex);
        for (auto &kv : g_ctx)
            if (std::find(devices.begin(), devices.end(), std::get<0>(kv.first)) == devices.end()) devices.push_back(std::get<0>(kv.first));
    }
    // Device by device, the device's lock first and the map's inside it - the order of on_device -> get_context: a call that
    // is using an engine finishes first, and a call that holds the device's lock never sees the map change under it
    // (chunk_engines looks its two engines up one after the other).
    for (int dev : devices)
        on_device(dev, 0, [&] {
            std::vector<ebcc_hip_ctx *> victims;
            {
                std::lock_guard<std::mutex> lock(g_map_mutex);
                for (auto i = g_ctx.begin(); i != g_ctx.end();)
                    if (std::get<0>(i->first) == dev) { victims.push_back(i->second); i = g_ctx.erase(i); } else ++i;
            }
            for (ebcc_hip_ctx *c : victims) ebcc_hip_destroy(c);
            return 0;
        });
    EBCC_API_CATCH_VOID
}

// The second engine set of a caller's context (made by the first shard / host-frames call of more than one batch: as much
// device memory as the context itself) is destroyed; the next such call makes it again.
void ebcc_hip_release_second_set(ebcc_hip_ctx *ctx)
{
    if (!ctx) return;
    on_device(ctx->device, 0, [&] {
        if (ctx->twin) { ebcc_hip_destroy(ctx->twin); ctx->twin = nullptr; }
        ctx->twin_failed = false;
        return 0;
    });
}

int ebcc_hip_prepare(ebcc_hip_ctx *ctx, size_t n_frames)
{
    if (!ctx || n_frames < 1 || n_frames > ctx->max_frames) { set_error("ebcc_hip_prepare: bad batch"); return 1; }
    return on_device(ctx->device, 1, [&] {
        slice_engines(ctx, n_frames, "EBCC_HIP_DECODE_SLICES", kDefaultDecodeSlices);                     // (the coarser slicing first:
        slice_engines(ctx, n_frames, "EBCC_HIP_SLICES", default_encode_slices());                        //  its lanes serve both)
        second_stream(ctx);
        for (ebcc_hip_ctx *c : ctx->lanes) second_stream(c);
        return 0;
    });
}

// One batch: the shard entry points below with at most the context's capacity of frames.
int ebcc_hip_encode_frames(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const codec_config_t *config,
                           uint8_t **out_streams, size_t *out_sizes)
{
    if (!ctx || n_frames < 1 || n_frames > ctx->max_frames) { set_error("ebcc_hip_encode_frames: bad batch"); return 1; }
    return encode_resident("ebcc_hip_encode_frames", ctx, d_frames, n_frames, config, out_streams, out_sizes);
}
int ebcc_hip_decode_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                           float *d_frames_out)
{
    return decode_resident("ebcc_hip_decode_frames", ctx, streams, sizes, n_frames, d_frames_out, DecodeRegion{}, true);
}

// Any number of frames resident on the device, coded in batches of the context's capacity on two alternating engine sets
// (GpuPhase above): the entropy stage of batch k runs beside the kernels of batch k + 1.  Same streams as
// ebcc_hip_encode_frames batch by batch.  On error every stream made so far is freed and the call returns 1.
int ebcc_hip_encode_shard(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const codec_config_t *config,
                          uint8_t **out_streams, size_t *out_sizes)
{
    return encode_resident("ebcc_hip_encode_shard", ctx, d_frames, n_frames, config, out_streams, out_sizes);
}

// ---- frame groups: many arrays of frames, a config each, in one call (encode_groups above)
long ebcc_hip_groups_check(size_t height, size_t width, const ebcc_hip_frame_group *groups, size_t n_groups)
{
    EBCC_API_TRY
    return groups_total("ebcc_hip_groups_check", height, width, groups, n_groups);
    EBCC_API_CATCH(-1)
}
int ebcc_hip_encode_frames_groups(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, uint8_t **out_streams, size_t *out_sizes)
{
    EBCC_API_TRY
    return encode_groups("ebcc_hip_encode_frames_groups", ctx, groups, n_groups, out_streams, out_sizes, GroupForm::Frames);
    EBCC_API_CATCH(1)
}
int ebcc_hip_encode_shard_groups(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, uint8_t **out_streams, size_t *out_sizes)
{
    EBCC_API_TRY
    return encode_groups("ebcc_hip_encode_shard_groups", ctx, groups, n_groups, out_streams, out_sizes, GroupForm::Shard);
    EBCC_API_CATCH(1)
}
int ebcc_hip_encode_host_frames_groups(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, uint8_t **out_streams, size_t *out_sizes)
{
    EBCC_API_TRY
    return encode_groups("ebcc_hip_encode_host_frames_groups", ctx, groups, n_groups, out_streams, out_sizes, GroupForm::Host);
    EBCC_API_CATCH(1)
}
int ebcc_hip_group_ranges(ebcc_hip_ctx *ctx, const float *const *d_ptrs, const size_t *n_floats, size_t n_groups, float *minmax, int *nonfinite)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_group_ranges";
    if (!ctx || !d_ptrs || !n_floats || !minmax || !nonfinite || n_groups < 1) { set_error("%s: bad arguments", who); return 1; }
    for (size_t g = 0; g < n_groups; g++)
        if (!d_ptrs[g] || n_floats[g] < 1 || ((uintptr_t) d_ptrs[g] & 3)) { set_error("%s: group %zu is empty or not 4-byte aligned", who, g); return 1; }
    return on_device(ctx->device, 1, [&] {
        std::vector<unsigned> keys(3 * n_groups);
        group_range_keys(ctx, d_ptrs, n_floats, n_groups, keys.data());
        int rc = 0;
        for (size_t g = 0; g < n_groups; g++) {
            nonfinite[g] = keys[3 * g + 2] != 0;
            if (nonfinite[g]) { if (!rc) set_error("%s: NaN or Inf found in the data of group %zu", who, g); rc = 2; continue; }
            minmax[2 * g] = float_of_order_key(keys[3 * g]); minmax[2 * g + 1] = float_of_order_key(keys[3 * g + 1]);
        }
        return rc;
    });
    EBCC_API_CATCH(1)
}

// ---- hard error bound (harden_batch above): the group entry points with the loop in every batch; one array is one group
int ebcc_hip_encode_shard_groups_hard(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, int max_rounds, uint8_t **out_streams,
                                      size_t *out_sizes, ebcc_hip_bound_report *report)
{
    EBCC_API_TRY
    const HardBound hard{max_rounds, report};
    return encode_groups("ebcc_hip_encode_shard_groups_hard", ctx, groups, n_groups, out_streams, out_sizes, GroupForm::Shard, &hard);
    EBCC_API_CATCH(1)
}
int ebcc_hip_encode_host_frames_groups_hard(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, int max_rounds,
                                            uint8_t **out_streams, size_t *out_sizes, ebcc_hip_bound_report *report)
{
    EBCC_API_TRY
    const HardBound hard{max_rounds, report};
    return encode_groups("ebcc_hip_encode_host_frames_groups_hard", ctx, groups, n_groups, out_streams, out_sizes, GroupForm::Host, &hard);
    EBCC_API_CATCH(1)
}
int ebcc_hip_encode_shard_hard(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const codec_config_t *config, int max_rounds,
                               uint8_t **out_streams, size_t *out_sizes, ebcc_hip_bound_report *report)
{
    EBCC_API_TRY
    if (!config) { set_error("ebcc_hip_encode_shard_hard: bad arguments"); return 1; }
    const ebcc_hip_frame_group one{d_frames, n_frames, *config, 0};
    const HardBound hard{max_rounds, report};
    return encode_groups("ebcc_hip_encode_shard_hard", ctx, &one, 1, out_streams, out_sizes, GroupForm::Shard, &hard);
    EBCC_API_CATCH(1)
}
int ebcc_hip_encode_host_frames_hard(ebcc_hip_ctx *ctx, const float *h_frames, size_t n_frames, const codec_config_t *config, int max_rounds,
                                     uint8_t **out_streams, size_t *out_sizes, ebcc_hip_bound_report *report)
{
    EBCC_API_TRY
    if (!config) { set_error("ebcc_hip_encode_host_frames_hard: bad arguments"); return 1; }
    const ebcc_hip_frame_group one{h_frames, n_frames, *config, 0};
    const HardBound hard{max_rounds, report};
    return encode_groups("ebcc_hip_encode_host_frames_hard", ctx, &one, 1, out_streams, out_sizes, GroupForm::Host, &hard);
    EBCC_API_CATCH(1)
}

// ---- audit (audit above): what the streams decode to against the originals, per frame
int ebcc_hip_frame_errors(ebcc_hip_ctx *ctx, const float *d_x, const float *d_d, size_t n_frames, size_t height, size_t width, const float *bound,
                          ebcc_hip_frame_error *report)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_frame_errors";
    size_t n_pix = 0;
    if (!ctx || !d_x || !d_d || !report || n_frames < 1 || ((uintptr_t) d_x & 3) || ((uintptr_t) d_d & 3) || height < 1 || width < 1 ||
        __builtin_mul_overflow(height, width, &n_pix) || n_pix > 0xFFFFFFFFu) { set_error("%s: bad arguments", who); return 1; }
    return on_device(ctx->device, 1, [&] {
        const int rc = frame_errors(ctx, d_x, d_d, n_frames, n_pix, bound, report);
        if (rc == 2) set_error("%s: NaN or Inf found in the originals", who);
        return rc;
    });
    EBCC_API_CATCH(1)
}
int ebcc_hip_audit_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const float *d_originals,
                          const float *bound, ebcc_hip_frame_error *report)
{
    EBCC_API_TRY
    return audit("ebcc_hip_audit_frames", ctx, streams, sizes, n_frames, d_originals, bound, report, AuditForm::Frames);
    EBCC_API_CATCH(1)
}
int ebcc_hip_audit_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const float *d_originals,
                         const float *bound, ebcc_hip_frame_error *report)
{
    EBCC_API_TRY
    return audit("ebcc_hip_audit_shard", ctx, streams, sizes, n_frames, d_originals, bound, report, AuditForm::Shard);
    EBCC_API_CATCH(1)
}
int ebcc_hip_audit_host_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const float *h_originals,
                               const float *bound, ebcc_hip_frame_error *report)
{
    EBCC_API_TRY
    return audit("ebcc_hip_audit_host_frames", ctx, streams, sizes, n_frames, h_originals, bound, report, AuditForm::Host);
    EBCC_API_CATCH(1)
}

// ---- reduce decode (reduce_shard above): statistics over time, folded on the device
long ebcc_hip_time_stats_check(size_t height, size_t width, const ebcc_hip_time_stats *stats, const uint32_t *bin, size_t n_frames, size_t row0,
                               size_t col0)
{
    EBCC_API_TRY
    return time_stats_named("ebcc_hip_time_stats_check", height, width, stats, bin, n_frames, row0, col0);
    EBCC_API_CATCH(-1)
}
int ebcc_hip_time_stats_init(ebcc_hip_ctx *ctx, const ebcc_hip_time_stats *stats)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_time_stats_init";
    if (!ctx) { set_error("%s: bad arguments", who); return 1; }
    if (!time_stats_shape(who, stats)) return 1;
    return start_values(ctx, {{stats->d_sum, 8, 0}, {stats->d_sum_sq, 8, 0}, {stats->d_over, 4, 0}, {stats->d_min, 4, kPlusInf}, {stats->d_max, 4, kMinusInf}},
                        stats->n_bins * stats->rows * stats->cols, stats->count, stats->n_bins);
    EBCC_API_CATCH(1)
}
int ebcc_hip_time_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, const uint32_t *bin, const ebcc_hip_time_stats *stats)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_time_fold";
    return items_call(who, ctx, {d_items}, n_items, [&] { return time_stats_named(who, stats ? stats->rows : 0, stats ? stats->cols : 0, stats, bin, n_items, 0, 0); }, [&] {
        time_fold(ctx, d_items, n_items, stats->rows * stats->cols, bin, *stats);
        count_named(n_items, bin, stats->count);
    });
    EBCC_API_CATCH(1)
}
int ebcc_hip_reduce_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin, size_t row0,
                          size_t col0, const ebcc_hip_time_stats *stats)
{
    EBCC_API_TRY
    return reduce_shard("ebcc_hip_reduce_shard", ctx, streams, sizes, n_frames, bin, row0, col0, stats);
    EBCC_API_CATCH(1)
}

// ---- area series (series_shard above): statistics over regions per frame, folded on the device
long ebcc_hip_area_check(size_t height, size_t width, const ebcc_hip_area_spec *spec, ebcc_hip_region *bounding)
{
    EBCC_API_TRY
    return area_checked("ebcc_hip_area_check", height, width, spec, bounding);
    EBCC_API_CATCH(-1)
}
int ebcc_hip_area_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, size_t height, size_t width, const ebcc_hip_area_spec *spec,
                       ebcc_hip_area_stat *out)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_area_fold";
    if (!ctx || !d_items || ((uintptr_t) d_items & 3) || !out || n_items < 1) { set_error("%s: bad arguments", who); return 1; }
    ebcc_hip_region bb{};
    if (area_checked(who, height, width, spec, &bb) < 0) return 1;
    size_t bytes = 0;
    if (__builtin_mul_overflow(n_items, spec->n_regions, &bytes) || __builtin_mul_overflow(bytes, sizeof(ebcc_hip_area_stat), &bytes) ||
        __builtin_mul_overflow(n_items, height * width * sizeof(float), &bytes)) { set_error("%s: the size of the items or of the records overflows", who); return 1; }
    return on_device(ctx->device, 1, [&] {
        if (spec->d_w_pix && area_weights_bad(ctx, spec->d_w_pix, width, bb)) { set_error("%s: d_w_pix holds a negative value, a NaN or an Inf", who); return 1; }
        area_fold(ctx, AreaItems{d_items, height * width, (unsigned) width, 0u, 0u}, n_items, height, width, *spec, out);
        return 0;
    });
    EBCC_API_CATCH(1)
}
int ebcc_hip_series_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_area_spec *spec,
                          ebcc_hip_area_stat *out)
{
    EBCC_API_TRY
    return series_shard("ebcc_hip_series_shard", ctx, streams, sizes, n_frames, spec, out);
    EBCC_API_CATCH(1)
}

// ---- regrid decode (regrid_shard above): decoded frames resampled by a separable map, on the device
long ebcc_hip_regrid_check(size_t height, size_t width, const ebcc_hip_regrid_spec *spec, ebcc_hip_region *bounding)
{
    EBCC_API_TRY
    return regrid_checked("ebcc_hip_regrid_check", height, width, spec, bounding);
    EBCC_API_CATCH(-1)
}
int ebcc_hip_regrid_items(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, size_t height, size_t width, const ebcc_hip_regrid_spec *spec,
                          float *d_out)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_regrid_items";
    if (!ctx || !d_items || ((uintptr_t) d_items & 3) || !d_out || ((uintptr_t) d_out & 3) || n_items < 1) { set_error("%s: bad arguments", who); return 1; }
    const long out_pix = regrid_checked(who, height, width, spec, nullptr);
    if (out_pix < 0) return 1;
    size_t bytes = 0;
    if (__builtin_mul_overflow(n_items, (size_t) out_pix * sizeof(float), &bytes) || __builtin_mul_overflow(n_items, height * width * sizeof(float), &bytes)) {
        set_error("%s: the size of the items or of the output overflows", who);
        return 1;
    }
    return on_device(ctx->device, 1, [&] {
        regrid_upload(ctx, *spec, ebcc_hip_region{0, 0, height, width});
        regrid_items(ctx, RegridItems{d_items, height * width, (unsigned) width, 0u, 0u}, n_items, width, *spec, d_out);
        return 0;
    });
    EBCC_API_CATCH(1)
}
int ebcc_hip_regrid_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_regrid_spec *spec,
                          float *d_out)
{
    EBCC_API_TRY
    return regrid_shard("ebcc_hip_regrid_shard", ctx, streams, sizes, n_frames, spec, d_out, false);
    EBCC_API_CATCH(1)
}
int ebcc_hip_regrid_host_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_regrid_spec *spec,
                                float *h_out)
{
    EBCC_API_TRY
    return regrid_shard("ebcc_hip_regrid_host_frames", ctx, streams, sizes, n_frames, spec, h_out, true);
    EBCC_API_CATCH(1)
}

// ---- quantile decode (quantile_shard above): order statistics over time, selected on the device
long ebcc_hip_time_ranks_check(size_t height, size_t width, const ebcc_hip_time_ranks *spec, const uint32_t *bin, size_t n_frames, size_t row0,
                               size_t col0)
{
    EBCC_API_TRY
    return time_ranks_named("ebcc_hip_time_ranks_check", height, width, spec, bin, n_frames, row0, col0);
    EBCC_API_CATCH(-1)
}
size_t ebcc_hip_time_ranks_work_bytes(const ebcc_hip_time_ranks *spec) { return time_ranks_work_bytes(spec); }
int ebcc_hip_rank_items(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, const uint32_t *bin, const ebcc_hip_time_ranks *spec)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_rank_items";
    RankPlan plan;
    return items_call(who, ctx, {d_items}, n_items, [&] { return time_ranks_named(who, spec ? spec->rows : 0, spec ? spec->cols : 0, spec, bin, n_items, 0, 0, &plan); }, [&] {
        rank_begin(ctx, plan);
        for (int pass = 0; pass < kRankPasses; pass++) {
            rank_count(ctx, plan, d_items, n_items, bin, pass);
            rank_advance(ctx, plan, pass, spec->d_out);
        }
        std::copy(plan.count.begin(), plan.count.end(), spec->count);
    });
    EBCC_API_CATCH(1)
}
int ebcc_hip_quantile_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin, size_t row0,
                            size_t col0, const ebcc_hip_time_ranks *spec)
{
    EBCC_API_TRY
    return quantile_shard("ebcc_hip_quantile_shard", ctx, streams, sizes, n_frames, bin, row0, col0, spec);
    EBCC_API_CATCH(1)
}

// ---- pair decode (pair_shard above): co-moments and vector magnitude of two variables over time, folded on the device
long ebcc_hip_pair_stats_check(size_t height, size_t width, const ebcc_hip_pair_stats *stats, const uint32_t *bin, size_t n_steps, size_t row0,
                               size_t col0)
{
    EBCC_API_TRY
    return pair_stats_named("ebcc_hip_pair_stats_check", height, width, stats, bin, n_steps, row0, col0);
    EBCC_API_CATCH(-1)
}
int ebcc_hip_pair_stats_init(ebcc_hip_ctx *ctx, const ebcc_hip_pair_stats *stats)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_pair_stats_init";
    if (!ctx) { set_error("%s: bad arguments", who); return 1; }
    if (!pair_stats_shape(who, stats)) return 1;
    return start_values(ctx, {{stats->d_sum_x, 8, 0}, {stats->d_sum_y, 8, 0}, {stats->d_sum_xx, 8, 0}, {stats->d_sum_yy, 8, 0}, {stats->d_sum_xy, 8, 0},
                              {stats->d_sum_mag, 8, 0}, {stats->d_over_mag, 4, 0}, {stats->d_max_mag, 4, kMinusInf}},
                        stats->n_bins * stats->rows * stats->cols, stats->count, stats->n_bins);
    EBCC_API_CATCH(1)
}
int ebcc_hip_pair_fold(ebcc_hip_ctx *ctx, const float *d_x_items, const float *d_y_items, size_t n_items, const uint32_t *bin,
                       const ebcc_hip_pair_stats *stats)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_pair_fold";
    return items_call(who, ctx, {d_x_items, d_y_items}, n_items, [&] { return pair_stats_named(who, stats ? stats->rows : 0, stats ? stats->cols : 0, stats, bin, n_items, 0, 0); }, [&] {
        pair_fold(ctx, d_x_items, d_y_items, false, n_items, stats->rows * stats->cols, bin, *stats);
        count_named(n_items, bin, stats->count);
    });
    EBCC_API_CATCH(1)
}
int ebcc_hip_pair_shard(ebcc_hip_ctx *ctx, const uint8_t *const *x_streams, const size_t *x_sizes, const uint8_t *const *y_streams,
                        const size_t *y_sizes, size_t n_steps, const uint32_t *bin, size_t row0, size_t col0, const ebcc_hip_pair_stats *stats)
{
    EBCC_API_TRY
    return pair_shard("ebcc_hip_pair_shard", ctx, x_streams, x_sizes, y_streams, y_sizes, n_steps, bin, row0, col0, stats);
    EBCC_API_CATCH(1)
}

// ---- spell decode (spell_shard above): run lengths and event timing over time, folded on the device
long ebcc_hip_spell_stats_check(size_t height, size_t width, const ebcc_hip_spell_stats *stats, const uint32_t *bin, const uint32_t *when,
                                size_t n_frames, size_t row0, size_t col0)
{
    EBCC_API_TRY
    return spell_stats_named("ebcc_hip_spell_stats_check", height, width, stats, bin, when, n_frames, row0, col0);
    EBCC_API_CATCH(-1)
}
int ebcc_hip_spell_stats_init(ebcc_hip_ctx *ctx, const ebcc_hip_spell_stats *stats)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_spell_stats_init";
    if (!ctx) { set_error("%s: bad arguments", who); return 1; }
    if (!spell_stats_shape(who, stats)) return 1;
    constexpr uint32_t no = EBCC_HIP_NO_STEP;
    return start_values(ctx, {{stats->d_run, 4, 0}, {stats->d_longest, 4, 0}, {stats->d_spells, 4, 0}, {stats->d_spell_steps, 4, 0}, {stats->d_events, 4, 0},
                              {stats->d_longest_end, 4, no}, {stats->d_first, 4, no}, {stats->d_last, 4, no}, {stats->d_when_min, 4, no}, {stats->d_when_max, 4, no},
                              {stats->d_min, 4, kPlusInf}, {stats->d_max, 4, kMinusInf}},
                        stats->n_bins * stats->rows * stats->cols, stats->count, stats->n_bins);
    EBCC_API_CATCH(1)
}
int ebcc_hip_spell_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, const uint32_t *bin, const uint32_t *when, const uint8_t *fresh,
                        const ebcc_hip_spell_stats *stats)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_spell_fold";
    return items_call(who, ctx, {d_items}, n_items, [&] { return spell_stats_named(who, stats ? stats->rows : 0, stats ? stats->cols : 0, stats, bin, when, n_items, 0, 0); }, [&] {
        spell_fold(ctx, d_items, n_items, stats->rows * stats->cols, bin, when, fresh, *stats);
        count_named(n_items, bin, stats->count);
    });
    EBCC_API_CATCH(1)
}
int ebcc_hip_spell_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin,
                         const uint32_t *when, const uint8_t *fresh, size_t row0, size_t col0, const ebcc_hip_spell_stats *stats)
{
    EBCC_API_TRY
    return spell_shard("ebcc_hip_spell_shard", ctx, streams, sizes, n_frames, bin, when, fresh, row0, col0, stats);
    EBCC_API_CATCH(1)
}

// ---- time-map decode (project_shard above): weighted sums over time, folded on the device
long ebcc_hip_time_map_check(size_t height, size_t width, const ebcc_hip_time_map *map, size_t n_frames, size_t row0, size_t col0)
{
    EBCC_API_TRY
    return time_map_named("ebcc_hip_time_map_check", height, width, map, n_frames, row0, col0);
    EBCC_API_CATCH(-1)
}
int ebcc_hip_time_map_init(ebcc_hip_ctx *ctx, const ebcc_hip_time_map *map)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_time_map_init";
    if (!ctx || !map || !map->d_acc || !map->count || ((uintptr_t) map->d_acc & 7)) { set_error("%s: bad arguments", who); return 1; }
    if (map->n_out < 1 || map->rows < 1 || map->cols < 1) { set_error("%s: n_out, rows and cols must not be zero", who); return 1; }
    if (!accumulator_bytes_checked(who, map->rows, map->cols, map->n_out, sizeof(double))) return 1;
    return start_values(ctx, {{map->d_acc, 8, 0}}, map->n_out * map->rows * map->cols, map->count, map->n_out);
    EBCC_API_CATCH(1)
}
int ebcc_hip_time_map_items(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, const ebcc_hip_time_map *map)
{
    EBCC_API_TRY
    const char *const who = "ebcc_hip_time_map_items";
    return items_call(who, ctx, {d_items}, n_items, [&] { return time_map_named(who, map ? map->rows : 0, map ? map->cols : 0, map, n_items, 0, 0); }, [&] {
        time_map(ctx, d_items, map->rows * map->cols, *map, 0, n_items, nullptr, 0);
        for (size_t o = 0; o < map->n_out; o++) map->count[o] += map->start[o + 1] - map->start[o];
    });
    EBCC_API_CATCH(1)
}
int ebcc_hip_project_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, size_t row0, size_t col0,
                           const ebcc_hip_time_map *map)
{
    EBCC_API_TRY
    return project_shard("ebcc_hip_project_shard", ctx, streams, sizes, n_frames, row0, col0, map);
    EBCC_API_CATCH(1)
}

// Any number of streams decoded to consecutive frames on the device, in batches of the context's capacity on the two
// engine sets side by side (decode_batches).  Same frames as ebcc_hip_decode_frames batch by batch.
int ebcc_hip_decode_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                          float *d_frames_out)
{
    return decode_resident("ebcc_hip_decode_shard", ctx, streams, sizes, n_frames, d_frames_out, DecodeRegion{}, false);
}

size_t ebcc_encode(float *data, codec_config_t *config, uint8_t **out_buffer)
{
    log_set_level_from_env();
    if (!dims_are_valid(config->dims)) {
        log_fatal("Invalid EBCC dimensions: product(dims[0..1]) and dims[2] must be between %d and %d",
                  EBCC_MIN_INTERNAL_IMAGE_DIM, EBCC_MAX_INTERNAL_IMAGE_DIM);
        return 0;
    }
    print_config(config);
    if (config->dims[0] != 1 && !tile_height_supported(config->dims[1])) {
        // the reference codes such a chunk as one tiled JPEG 2000 image (src/ebcc_codec.c:121-125,167-171) and crashes
        // inside OpenJPEG when the tiles are too small for 6 resolutions
        log_fatal("chunks holding %lu frames of %lu rows are not supported (a chunk of several frames is a tiled JPEG 2000 "
                  "image: tiles need at least 32 rows)", config->dims[0], config->dims[1]);
        return 0;
    }
    size_t size = 0;
    uint8_t *o = nullptr;
    const int rcode = encode_on_device(resolve_device(), data, 1, (int) config->dims[1], (int) config->dims[2], config, &o, &size, config->dims[0]);
    if (rcode == 2) exit(1);                                                                   // check_nan_inf, :598-605
    if (rcode) { free(o); return 0; }
    *out_buffer = o;
    return size;
}

size_t ebcc_decode(uint8_t *data, size_t data_size, float **out_buffer)
{
    ParsedFrame hd;                                                                             // both stream formats
    if (!parse_frame(data, data_size, hd)) return 0;
    const uint8_t *tail = hd.tail;
    if (hd.const_field) {                                                                      // :1265-1281 / :1175-1183, no device work
        uint64_t cnt;
        memcpy(&cnt, tail, 8);
        float *o = (float *) malloc(cnt * sizeof(float));
        if (!o) { log_fatal("out of memory"); return 0; }
        for (uint64_t i = 0; i < cnt; i++) o[i] = hd.minv;
        *out_buffer = o;
        return (size_t) cnt;
    }
    int H = 0, W = 0, tw = 0, th = 0;
    if (!j2k_peek_dims(tail, hd.tail_size, &W, &H, &tw, &th) || H < 1 || W < 1 || H > 2047 || W > 2047 || th < 1 || tw != W || H % th != 0) {
        log_fatal("Invalid encoded data: no usable JPEG 2000 codestream in the tail");
        return 0;
    }
    const size_t tiles = (size_t) (H / th);
    if (tiles > 1 && !tile_height_supported((size_t) th)) {
        log_fatal("streams with %zu tiles of %d rows are not supported", tiles, th);
        return 0;
    }
    const int device = resolve_device();
    // (no libzstd needed here for a stream without a residual layer: decode_batch asks for it when there is one)
    return on_device(device, (size_t) 0, [&]() -> size_t {
        ebcc_hip_ctx *ctx = nullptr, *rc = nullptr;
        if (!chunk_engines(device, th, W, 1, tiles, &ctx, &rc)) return 0;
        const size_t n_pix = (size_t) H * W;
        PhaseTimer pt;
        float *d = io_buffer(ctx, n_pix * sizeof(float));
        const uint8_t *sp = data;
        if (decode_batch(ctx, &sp, &data_size, 1, d, nullptr, tiles, rc)) return 0;
        pt.mark("ebcc_decode: decode_batch");
        // :1126-1128: honour a caller-provided buffer
        float *o = *out_buffer ? *out_buffer : (float *) malloc(n_pix * sizeof(float));
        if (!o) { log_fatal("out of memory"); return 0; }
        EBCC_HIP_CHECK(hipMemcpy(o, d, n_pix * sizeof(float), hipMemcpyDeviceToHost));
        pt.mark("ebcc_decode: download");
        *out_buffer = o;
        return n_pix;
    });
}

// ---- EBCK chunk container (the reference's src/ebcc_codec.c:920-1052) -------------------------------------------------------------
size_t ebcc_encode_chunking(float *data, codec_config_t *config, uint8_t **out_buffer)
{
    log_set_level_from_env();
    size_t cd[3];
    bool all_zero = true;
    for (int i = 0; i < 3; i++) { cd[i] = config->chunk_dims[i]; if (cd[i]) all_zero = false; }
    if (all_zero) for (int i = 0; i < 3; i++) cd[i] = config->dims[i];
    if (!dims_are_valid(cd)) {
        log_fatal("Invalid chunking dimensions: product(chunk_dims[0..1]) and chunk_dims[2] must be between %d and %d",
                  EBCC_MIN_INTERNAL_IMAGE_DIM, EBCC_MAX_INTERNAL_IMAGE_DIM);
        return 0;
    }
    size_t cnt[3];
    for (int i = 0; i < 3; i++) {
        if (config->dims[i] == 0 || cd[i] == 0) { log_fatal("Invalid chunking dimensions: dims and chunk_dims must be non-zero"); return 0; }
        cnt[i] = cdiv(config->dims[i], cd[i]);
    }
    if (cd[0] != 1 && !tile_height_supported(cd[1])) {
        log_fatal("chunks holding %lu frames of %lu rows are not supported (a chunk of several frames is a tiled JPEG 2000 "
                  "image: tiles need at least 32 rows); use chunk_dims[0] = 1", cd[0], cd[1]);
        return 0;
    }
    const size_t csize = cd[0] * cd[1] * cd[2], nchunks = cnt[0] * cnt[1] * cnt[2];
    const size_t total = config->dims[0] * config->dims[1] * config->dims[2];
    const size_t padded = csize * nchunks;
    if (padded > total && padded - total > total / 10)
        log_warn("Chunk padding adds %lu values over %lu real values (%.2f%%)", padded - total, total,
                 ((double) (padded - total) / (double) total) * 100.0);
    // the chunks in C order of chunk index (:311-318), edge chunks padded by index clamping (:339-351).  Chunks that
    // are whole frames of the array need no copy at all.
    ChunkBox box;
    for (int i = 0; i < 3; i++) { box.dims[i] = config->dims[i]; box.cd[i] = cd[i]; box.cnt[i] = cnt[i]; }
    bool in_place = box.slabs();
    for (size_t cl = 0; cl < nchunks && in_place; cl++) in_place = box.inside(cl);
    std::vector<float> gathered;
    if (!in_place) {
        gathered.resize(nchunks * csize);
        for (size_t cl = 0; cl < nchunks; cl++) box.gather(data, cl, gathered.data() + cl * csize);
    }
    const float *chunk_data = in_place ? data : gathered.data();
    codec_config_t cc = *config;
    for (int i = 0; i < 3; i++) { cc.dims[i] = cd[i]; cc.chunk_dims[i] = 0; }
    std::vector<uint8_t *> outs(nchunks, nullptr);
    std::vector<size_t> sizes(nchunks, 0);
    const int rcode = run_on_devices(nchunks, [&](int device, size_t first, size_t count) {
        return encode_on_device(device, chunk_data + first * csize, count, (int) cd[1], (int) cd[2], &cc, outs.data() + first, sizes.data() + first, cd[0]);
    });
    if (rcode == 2) exit(1);                                                                   // check_nan_inf, :598-605
    if (rcode) {
        for (auto p : outs) free(p);
        return 0;
    }
    size_t len = 0;
    uint8_t *o = assemble_container(config->dims, cd, nchunks, csize, outs.data(), sizes.data(), &len);
    for (auto q : outs) free(q);
    if (!o) return 0;
    *out_buffer = o;
    return len;
}

size_t ebcc_encode_chunking_compat(float *data, codec_config_t *config, uint8_t **out_buffer)
{
    // :1054-1090
    log_set_level_from_env();
    codec_config_t c = *config;
    if (!c.chunk_dims[0] && !c.chunk_dims[1] && !c.chunk_dims[2]) {
        c.chunk_dims[0] = 1;
        c.chunk_dims[1] = c.dims[1] > EBCC_MAX_INTERNAL_IMAGE_DIM ? 1024 : c.dims[1];
        c.chunk_dims[2] = c.dims[2] > EBCC_MAX_INTERNAL_IMAGE_DIM ? 1024 : c.dims[2];
        log_info("ebcc_encode_chunking_compat chunk dimensions: (%lu, %lu, %lu)", c.chunk_dims[0], c.chunk_dims[1], c.chunk_dims[2]);
    }
    if (c.residual_compression_type == RELATIVE_ERROR) {
        size_t total = c.dims[0] * c.dims[1] * c.dims[2];
        if (total == 0) { log_fatal("Invalid EBCC dimensions: size overflow or zero-sized data"); return 0; }
        float mn = data[0], mx = data[0];
        for (size_t i = 0; i < total; i++) {
            if (std::isnan(data[i]) || std::isinf(data[i])) { log_fatal("NaN or Inf found in data at index %lu", i); exit(1); }
            if (data[i] > mx) mx = data[i];
            if (data[i] < mn) mn = data[i];
        }
        c.error *= mx - mn;                                                                    // global range, :1085
        c.residual_compression_type = MAX_ERROR;
    }
    return ebcc_encode_chunking(data, &c, out_buffer);
}

size_t ebcc_decode_chunking(uint8_t *data, size_t data_size, float **out_buffer)
{
    // :1322-1449
    log_set_level_from_env();
    if (data_size < sizeof(ChunkHeader) || memcmp(data, EBCC_CHUNKING_HEADER_MAGIC, 4) != 0) return ebcc_decode(data, data_size, out_buffer);
    Container held;
    const std::string bad = held.parse(data, data_size);
    if (!bad.empty()) { log_fatal("%s", bad.c_str()); return 0; }
    const size_t *const dims = held.dims, *const cd = held.cd, *const cnt = held.cnt;
    const size_t csize = held.csize, nchunks = held.nchunks, total = held.total;
    const std::vector<const uint8_t *> &ptrs = held.ptrs;
    const std::vector<size_t> &lens = held.lens;
    const int H = (int) cd[1], W = (int) cd[2];
    ChunkBox box;
    for (int i = 0; i < 3; i++) { box.dims[i] = dims[i]; box.cd[i] = cd[i]; box.cnt[i] = cnt[i]; }
    bool in_place = box.slabs();                               // chunks = whole frames of the array: decode straight into it
    for (size_t cl = 0; cl < nchunks && in_place; cl++) in_place = box.inside(cl);
    float *o = (float *) malloc(total * sizeof(float));
    if (!o) { log_fatal("Failed to allocate chunked EBCC decode output"); return 0; }
    std::vector<float> chunks;
    if (!in_place) chunks.resize(nchunks * csize);
    float *h_chunks = in_place ? o : chunks.data();
    // (the reference-compatible output must be a malloc'd buffer: its pages are mapped while the GPU decodes)
    Prefault prefault(in_place ? (void *) o : nullptr, in_place ? total * sizeof(float) : 0);
    const size_t tiles = cd[0];
    const int rcode = run_on_devices(nchunks, [&](int device, size_t first, size_t count) {
        return on_codec(device, 1, [&] {
            const size_t cap = std::min(count, batch_capacity(csize, tiles));
            ebcc_hip_ctx *ctx = nullptr, *rc = nullptr;
            if (!chunk_engines(device, H, W, cap, tiles, &ctx, &rc)) return 1;
            return decode_to_host(ctx, rc, tiles, cap, ptrs.data() + first, lens.data() + first, count, h_chunks + first * csize, &prefault);
        });
    });
    if (rcode) { prefault.join(); free(o); return 0; }         // (the page-touching threads write into `o` until they are joined)
    if (!in_place)
        for (size_t cl = 0; cl < nchunks; cl++) box.scatter(chunks.data() + cl * csize, cl, o);          // :353-370
    *out_buffer = o;
    return total;
}

// The slab of a container on the cached engines of one device (include/ebcc_hip.h): the chunks it meets through decode_to_host
// as placed boxes of a compact [nt][rows][cols] array.
size_t ebcc_decode_chunking_slab(uint8_t *data, size_t data_size, const ebcc_hip_slab *slab, float **out_buffer)
{
    EBCC_API_TRY
    const char *const who = "ebcc_decode_chunking_slab";
    log_set_level_from_env();
    Container held;
    std::vector<ebcc_hip_placed_box> boxes;
    if (!out_buffer) { set_error("%s: bad arguments", who); return 0; }
    if (!slab_boxes(who, held, data, data_size, slab, 0, 0, boxes)) { log_fatal("%s", ebcc_hip_last_error()); return 0; }
    const size_t floats = slab->nt * slab->rows * slab->cols;
    float *o = (float *) malloc(floats * sizeof(float));
    if (!o) { log_fatal("Failed to allocate chunked EBCC decode output"); return 0; }
    const int H = (int) held.cd[1], W = (int) held.cd[2], device = resolve_device();
    const int rcode = on_codec(device, 1, [&] {
        ebcc_hip_ctx *ctx = nullptr, *rc = nullptr;
        if (!chunk_engines(device, H, W, std::min(boxes.size(), batch_capacity(held.csize)), 1, &ctx, &rc)) return 1;
        DecodeRegion region = DecodeRegion::placed_list(boxes.data(), boxes.size(), floats);
        const uint8_t *const *streams = held.ptrs.data();
        const size_t *sizes = held.lens.data();
        size_t n = held.nchunks;
        BoxCall call;
        if (decode_region(who, ctx, streams, sizes, n, region, call)) return 1;
        return decode_to_host(ctx, nullptr, 1, ctx->max_frames, streams, sizes, n, o, nullptr, region);
    });
    if (rcode) { free(o); return 0; }
    *out_buffer = o;
    return floats;
    EBCC_API_CATCH(0)
}

}  // extern "C"
