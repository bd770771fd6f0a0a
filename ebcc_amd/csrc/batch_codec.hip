// batch_codec.hip - one device batch of the frame codec (host.hpp): /root/reference/src/ebcc_codec.c:607-918 as
// encode_batch, :1215-1320 as decode_batch - chunks of one frame or of several (Batch) either way - with the rate search
// (:545-596, twice per frame) and the truncation bisection (:765-796) as device-side state machines (search.hpp).  The
// host only steers: per-frame scalars come back from the device after every search, every per-sample operation runs in
// the kernels.
#include "host.hpp"

namespace ebcc {
namespace {

// rate search k's state before its first round (:545-596 entered at rate cr0 with the quantile q_init of a probe there):
// phase 0, nothing pending, no probe asked for, no final probe yet
DevRateSearch rate_search_start(float cr0, double q_init, double q_target)
{
    DevRateSearch r{};
    r.lo = r.hi = r.cr = cr0; r.q = r.q0 = q_init; r.qt = q_target;
    r.last.cr = -1; r.last.complete = 1;
    return r;
}

struct Job {                     // host-side state of one frame being encoded
    FrameConfig fc;              // its rate, mode and bound
    bool const_field = false;
    bool search = false;         // it runs the searches and the residual layer: an error-bounded mode, not constant
    float minv = 0, maxv = 0, target = -1, cr = -1;
    double mean_err = 0, q = 0, q_first = 0;
    float rmin = 0, rmax = 0;
    bool skip = true, need_pure = false;
    float best_err = -1;
    size_t coeffs_orig = 0, coeffs_size = 0, len1 = 0;
    double t_hi = 0, t_lo = 0, t_best = 0;
    bool trunc_active = false;
    std::vector<uint8_t> tail, zbytes;
    // rate searches: [0] error-bounded (:728), [1] pure base layer (:836), in the device's layout; rs[k].last is the probe
    // search k's result rests on.  A probe's outcome depends only on (frame, rate), so both searches share one record of
    // the probes made so far.
    DevRateSearch rs[2] = {};
    std::vector<DevProbe> probes;
};

// The base layer of a batch of chunks.  A chunk is one frame, or `tiles` frames stacked along the row axis that
// the reference codes as ONE JPEG 2000 image with one tile per frame (src/ebcc_codec.c:105-180, n_tiles > 1).
// Every tile is a frame of the engine `ctx` (tile t of chunk c at index c * tiles + t); the arrays below are per
// CHUNK - rate, target, error statistics, codestream size - and are expanded to / gathered from the tiles here:
//   * all tiles of a chunk are probed at the same rate; a tile's byte budget subtracts its share of the main
//     header only (opj_j2k_update_rates: 135 / tiles, J2kFrame::hdr_share);
//   * nbad / err_sum add up; the codestream is main header (SIZ rewritten for the stacked image) + the tile-parts
//     (SOT with the tile index) + EOC, byte-identical to OpenJPEG's opj_write_tile sequence.
// The residual layer works on whole chunks in the engine `rc` (== ctx for one-frame chunks).
struct Batch {
    ebcc_hip_ctx *ctx;
    J2kBuffers &jb;
    const float *d_frames;
    size_t n, tiles, nt;           // chunks, tiles per chunk, n * tiles
    std::vector<J2kFrame> jf;      // per chunk
    J2kFrame *tjf;                 // per tile (device image; pinned: ctx->h_jf)
    std::vector<int> active;       // per chunk
    int *tactive, *ractive;        // pinned: ctx->h_act
    std::vector<float> state_cr;   // rate of the decode the engine holds for every chunk (-1: none)
    int *d_active;                 // per tile, on ctx
    hipStream_t s;
    ebcc_hip_ctx *rc;              // residual engine (chunk-sized frames)
    hipStream_t rs;
    Batch(ebcc_hip_ctx *c, const float *d, size_t n_, size_t tiles_ = 1, ebcc_hip_ctx *rc_ = nullptr)
        : ctx(c), jb(*static_cast<J2kBuffers *>(c->j2k)), d_frames(d), n(n_), tiles(tiles_), nt(n_ * tiles_), jf(n_),
          tjf(static_cast<J2kFrame *>(c->h_jf)), active(n_, 0), tactive(c->h_act), ractive(c->h_act + c->max_frames), state_cr(n_, -1.f),
          d_active(c->d_active), s(c->stream), rc(rc_ ? rc_ : c), rs((rc_ ? rc_ : c)->stream)
    {
        memset(tjf, 0, sizeof(J2kFrame) * nt);
    }
    void fetch_jf(hipStream_t on = nullptr)
    {
        if (!on) on = s;
        EBCC_HIP_CHECK(hipMemcpyAsync(tjf, jb.jf, sizeof(J2kFrame) * nt, hipMemcpyDeviceToHost, on));
        wait_stream(on);
        for (size_t c = 0; c < n; c++) {
            J2kFrame &o = jf[c];
            o.nbad = 0; o.err_sum = 0; o.overflow = 0; o.body_bytes = 0;
            for (size_t t = c * tiles; t < (c + 1) * tiles; t++) {
                o.nbad += tjf[t].nbad; o.err_sum += tjf[t].err_sum; o.overflow |= tjf[t].overflow; o.body_bytes += tjf[t].body_bytes;
            }
            o.stream_bytes = kJ2kMainHeaderBytes + (int) tiles * 14 + o.body_bytes + 2;     // main header, SOT + SOD per tile, EOC
        }
    }
    void push_jf()
    {
        for (size_t c = 0; c < n; c++)
            for (size_t t = c * tiles; t < (c + 1) * tiles; t++) {
                tjf[t].cr = jf[c].cr; tjf[t].target = jf[c].target;
                tjf[t].hdr_share = tiles > 1 ? (float) kJ2kMainHeaderBytes / (float) tiles : 0.0f;
            }
        EBCC_HIP_CHECK(hipMemcpyAsync(jb.jf, tjf, sizeof(J2kFrame) * nt, hipMemcpyHostToDevice, s));
    }
    void push_active()
    {
        for (size_t c = 0; c < n; c++)
            for (size_t t = c * tiles; t < (c + 1) * tiles; t++) tactive[t] = active[c];
        EBCC_HIP_CHECK(hipMemcpyAsync(d_active, tactive, sizeof(int) * nt, hipMemcpyHostToDevice, s));
    }
    // the chunk mask for the residual engine's kernels
    void push_ractive()
    {
        for (size_t c = 0; c < n; c++) ractive[c] = active[c];
        EBCC_HIP_CHECK(hipMemcpyAsync(rc->d_active, ractive, sizeof(int) * n, hipMemcpyHostToDevice, rs));
    }
    // the layer assignment of the active chunks at rate jf[c].cr
    void allocate()
    {
        push_jf();
        push_active();
        launch_j2k_rate(jb, (int) nt, d_active, s);
    }
    // codestream of the current layer assignment of the active chunks -> jobs[c].tail
    template <class Jobs>
    void collect_tails(Jobs &jobs)
    {
        push_active();
        launch_j2k_write(jb, (int) nt, d_active, s);
        fetch_jf();
        if (tiles == 1) {
            // all codestreams of the batch in one packed download (engine.hip: stage_download)
            std::vector<size_t> len(n, 0), off(n, 0);
            for (size_t f = 0; f < n; f++) if (active[f]) len[f] = (size_t) jf[f].stream_bytes;
            stage_download(ctx, jb.stream, jb.stream_cap, len.data(), off.data(), n, s);
            for (size_t f = 0; f < n; f++)
                if (active[f]) jobs[f].tail.assign(ctx->h_stage + off[f], ctx->h_stage + off[f] + len[f]);
            return;
        }
        // every tile was written as a one-tile codestream into its slot: [main header 135][SOT 12][SOD 2][packets][EOC 2]
        for (size_t c = 0; c < n; c++) {
            if (!active[c]) continue;
            std::vector<uint8_t> &o = jobs[c].tail;
            o.resize((size_t) jf[c].stream_bytes);
            size_t at = kJ2kMainHeaderBytes;
            for (size_t k = 0; k < tiles; k++) {
                const size_t t = c * tiles + k, part = 14 + (size_t) tjf[t].body_bytes;
                const uint8_t *slot = jb.stream + t * jb.stream_cap;
                if (k == 0) EBCC_HIP_CHECK(hipMemcpyAsync(o.data(), slot, kJ2kMainHeaderBytes, hipMemcpyDeviceToHost, s));
                EBCC_HIP_CHECK(hipMemcpyAsync(o.data() + at, slot + kJ2kMainHeaderBytes, part, hipMemcpyDeviceToHost, s));
                at += part;
            }
        }
        wait_stream(s);
        const unsigned H = (unsigned) jb.geom.H;
        for (size_t c = 0; c < n; c++) {
            if (!active[c]) continue;
            std::vector<uint8_t> &o = jobs[c].tail;
            auto put32 = [&](size_t at, unsigned v) { o[at] = (uint8_t) (v >> 24); o[at + 1] = (uint8_t) (v >> 16); o[at + 2] = (uint8_t) (v >> 8); o[at + 3] = (uint8_t) v; };
            put32(12, H * (unsigned) tiles);                             // SIZ: Ysiz (tile size XTsiz/YTsiz stays W x H)
            size_t at = kJ2kMainHeaderBytes;
            for (size_t k = 0; k < tiles; k++) {
                o[at + 4] = (uint8_t) (k >> 8); o[at + 5] = (uint8_t) k;  // SOT: Isot
                at += 14 + (size_t) tjf[c * tiles + k].body_bytes;
            }
            o[at] = 0xFF; o[at + 1] = 0xD9;                               // EOC
        }
    }
};

int search_rounds() { const char *e = getenv("EBCC_HIP_SEARCH_ROUNDS"); return e ? std::max(1, atoi(e)) : 16; }
constexpr int kSearchAll = 0, kSearchStart = 1, kSearchFinish = 2;

// The entropy stage of a batch (:811-817): level-22 zstd of the kept SPIHT prefixes and lower bounds of their compressed
// sizes (zstd_size_lower_bound), as jobs on the process-wide pool (HostPool) - every slice of a batch feeds the same
// workers, so the host is never oversubscribed however many slices run.  The workers write into the batch's jobs and
// hold `this`: an Entropy lives inside the jobs' lifetime, stays where it is, and waits for its jobs when it goes (error
// paths too).
struct Entropy {
    enum : uint8_t { kNone = 0, kQueued = 1, kRunning = 2, kSkipped = 3 };
    using PoolBatches = std::vector<std::shared_ptr<HostPool::Batch>>;
    std::vector<Job> &jobs;
    const unsigned slices;
    const int level;
    const bool timing, trace;                                       // EBCC_HIP_PHASE_TIMING; EBCC_HIP_ZSTD_TRACE as well
    std::vector<const uint8_t *> coeff_ptr;                         // the kept prefix of a frame in pinned host memory
    std::unique_ptr<std::atomic<uint8_t>[]> zstate;
    std::vector<size_t> zfloor;                                     // lower bound of z (0: none)
    std::atomic<long long> zstd_us{0}, zstd_max_us{0}, zstd_bytes{0}, bound_us{0};    // core time, longest job, bytes
    long long wait_us = 0;
    PoolBatches zbatches, fbatches;                                 // level-22 jobs; lower bounds

    Entropy(std::vector<Job> &j, unsigned slices_, int level_, bool timing_)
        : jobs(j), slices(slices_), level(level_), timing(timing_), trace(timing_ && getenv("EBCC_HIP_ZSTD_TRACE")),
          coeff_ptr(j.size(), nullptr), zstate(new std::atomic<uint8_t>[j.size()]), zfloor(j.size(), 0)
    { for (size_t f = 0; f < j.size(); f++) zstate[f] = kNone; }
    Entropy(const Entropy &) = delete; Entropy &operator=(const Entropy &) = delete;
    ~Entropy() { for (PoolBatches *v : {&fbatches, &zbatches}) for (auto &b : *v) if (b) b->wait(); }

    // level-22 zstd of the frames in `list`, in the order given; a frame that was decided in the meantime (kSkipped) is
    // passed over
    void submit_zstd(std::vector<size_t> list)
    {
        if (trace) fprintf(stderr, "zstd-submit batch %p jobs %zu\n", (const void *) &jobs, list.size());
        for (size_t f : list) zstate[f] = kQueued;
        auto order = std::make_shared<std::vector<size_t>>(std::move(list));
        zbatches.push_back(HostPool::instance().submit(order->size(), entropy_threads(slices), [this, order](size_t i) {
            const size_t f = (*order)[i];
            uint8_t expect = kQueued;
            if (!zstate[f].compare_exchange_strong(expect, kRunning)) return;
            Job &j = jobs[f];
            const auto z0 = std::chrono::steady_clock::now();
            j.zbytes.resize(zstd().bound(j.coeffs_size));
            const size_t z = zstd().compress(j.zbytes.data(), j.zbytes.size(), coeff_ptr[f], j.coeffs_size, level);
            if ((zstd().is_error && zstd().is_error(z)) || z > j.zbytes.size()) throw std::runtime_error("ZSTD_compress failed on a residual prefix");
            j.zbytes.resize(z);
            const long long us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - z0).count();
            if (trace) {                                                // (when each job ran, on which CPU)
                static const auto epoch = std::chrono::steady_clock::now();
                const long long a = std::chrono::duration_cast<std::chrono::microseconds>(z0 - epoch).count();
                fprintf(stderr, "zstd-job batch %p bytes %zu start %lld us end %lld us cpu %d\n", (const void *) &jobs, j.coeffs_size, a, a + us, sched_getcpu());
            }
            zstd_us += us; zstd_bytes += (long long) j.coeffs_size;
            long long m = zstd_max_us.load(); while (us > m && !zstd_max_us.compare_exchange_weak(m, us)) {}
        }));
    }
    // the lower bounds of z for the frames in `frames`
    void submit_floors(const std::vector<size_t> &frames)
    {
        auto list = std::make_shared<std::vector<size_t>>(frames);
        fbatches.push_back(HostPool::instance().submit(list->size(), entropy_threads(slices), [this, list](size_t i) {
            const size_t f = (*list)[i];
            const auto z0 = std::chrono::steady_clock::now();
            zfloor[f] = zstd_size_lower_bound(coeff_ptr[f], jobs[f].coeffs_size);
            bound_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - z0).count();
        }));
    }
    // longest first: level 22 takes ~0.2 ms per KB on one core and a batch has frames whose prefix is ten times the
    // average - started last, such a frame alone decides when the slice can go on
    std::vector<size_t> longest_first(std::vector<size_t> list) const
    {
        std::stable_sort(list.begin(), list.end(), [&](size_t a, size_t c) { return jobs[a].coeffs_size > jobs[c].coeffs_size; });
        return list;
    }
    // lowest floor per byte first: the order in which the frames are likely to need their z
    std::vector<size_t> lowest_floor_first(std::vector<size_t> list) const
    {
        std::stable_sort(list.begin(), list.end(), [&](size_t a, size_t c) {
            return (double) zfloor[a] * (double) jobs[c].coeffs_size < (double) zfloor[c] * (double) jobs[a].coeffs_size; });
        return list;
    }
    std::vector<size_t> not_started(std::vector<size_t> v) const   // (frames already queued or decided are dropped)
    {
        v.erase(std::remove_if(v.begin(), v.end(), [&](size_t f) { return zstate[f] != kNone; }), v.end());
        return v;
    }
    // z >= zfloor: len2 < zfloor + len1 implies len2 < z + len1 - the base layer alone wins (:838), whatever z is
    bool floor_decides(size_t f) const { return zfloor[f] > 0 && (size_t) jobs[f].rs[1].last.stream_bytes < zfloor[f] + jobs[f].len1; }
    // a frame decided before a worker took it up (not queued yet, or queued on the speculative list) is not compressed
    bool strike(size_t f)
    {
        uint8_t expect = kNone;
        if (zstate[f].compare_exchange_strong(expect, kSkipped)) return true;
        expect = kQueued;
        return zstate[f].compare_exchange_strong(expect, kSkipped);
    }
    bool join(PoolBatches &v)
    {
        const auto w0 = std::chrono::steady_clock::now();
        bool ok = true;
        std::string why;
        for (auto &b : v) if (b && !b->wait()) { ok = false; if (why.empty()) why = b->error; }
        v.clear();
        wait_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - w0).count();
        if (!ok) { log_fatal("entropy stage failed: %s", why.c_str()); set_error("%s", why.c_str()); }
        return ok;
    }
    bool join_floors() { return join(fbatches); }
    bool join_all() { const bool a = join(fbatches), c = join(zbatches); return a && c; }
    // the stage's totals (EBCC_HIP_PHASE_TIMING) and every prefix's sizes and fate (EBCC_HIP_ZSTD_TRACE)
    void report(const std::vector<size_t> &with_prefix, long long skipped, long long skipped_bytes) const
    {
        if (timing) fprintf(stderr, "ebcc-mi355x zstd: %.1f ms of core time for %lld bytes, longest job %.1f ms; floors %.1f ms; %lld of %zu prefixes (%lld bytes) not compressed\n",
                            zstd_us.load() / 1e3, zstd_bytes.load(), zstd_max_us.load() / 1e3, bound_us.load() / 1e3, skipped, with_prefix.size(), skipped_bytes);
        host_stats().skipped_bytes += skipped_bytes;
        if (trace)
            for (size_t f : with_prefix) {
                const Job &j = jobs[f];
                const long long x = (long long) j.rs[1].last.stream_bytes - (long long) j.len1;
                fprintf(stderr, "zstd-trace c %zu floor %zu X %lld z %zu state %d need_pure %d nbad1 %llu len1 %zu orig %zu\n", j.coeffs_size, zfloor[f], x, j.zbytes.size(), (int) zstate[f].load(), (int) j.need_pure,
                        (unsigned long long) j.rs[0].last.nbad, j.len1, j.coeffs_orig);
            }
    }
};

// One call of encode_batch: the batch, the jobs of its chunks and what every phase reads.  The phases are the steps of
// the reference's ebcc_encode in its order, each headed by the lines it restates; their host synchronisations, uploads
// and launches are the slice schedule the codec was measured with.
// Rate, mode and bound are per chunk (Job::fc: a batch of frame groups mixes them; the environment switches stay
// process-wide).  A phase runs when a chunk needs it, and a chunk that does not need it is inactive in it the way a constant
// chunk is (active[f] = 0, rs[k].phase = 6): a chunk in mode NONE takes the first probe's allocation without its decode and
// hands its codestream over there, one with a stale mode value does so behind the decode (quirk Q2), and everything from
// search #1 on - the residual range, both searches, the residual layer, the truncation search, the entropy stage and the
// :838 comparison - sees the searching chunks (Job::search) alone.  With one config for all chunks these are the masks and
// the launches of the uniform encoder.
struct BatchEncode {
    struct Gate { SliceGate *g; void release() { if (g) { g->release(); g = nullptr; } } ~Gate() { release(); } } next;   // (error paths too)
    struct NoteOnce { PhaseNote *n; void tell() { if (n) { n->slice_done(); n = nullptr; } } ~NoteOnce() { tell(); } } gpu_phase_over;   // (every path reports once)
    const EncodeEnv env;
    const double q_target;
    const bool want_pure;                                           // the pure base-layer fallback runs (:738)
    const size_t n, n_pix;                                          // chunks, pixels of a chunk
    const unsigned slices;
    Batch b;
    const bool overlap2;                                            // search #2 beside the residual layer (queue_search_2)
    std::vector<Job> jobs;
    PhaseTimer pt;
    bool any_search = false;                                        // a chunk runs the searches (Job::search): the phases behind the first probe run
    bool any_resid = false;                                         // a chunk needs the residual layer
    bool search2_queued = false;                                    // rounds of search #2 are in flight on the second stream

    BatchEncode(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_, const FrameConfig *fc, SliceGate *next_, size_t tiles,
                ebcc_hip_ctx *rctx, unsigned slices_, PhaseNote *note)
        : next{next_}, gpu_phase_over{note}, q_target(1 - env.base_error_quantile),
          want_pure(q_target != 1.0 && !env.no_fallback), n(n_), n_pix(ctx->n_pix * tiles), slices(slices_),
          b(ctx, d_frames, n_, tiles, rctx), overlap2(want_pure && tiles == 1 && b.rc == ctx), jobs(n_)
    { for (size_t f = 0; f < n; f++) jobs[f].fc = fc[f]; }
    // an error return between the two halves of search #2 must not leave its rounds in flight
    ~BatchEncode() { if (search2_queued && b.ctx->stream2) hipStreamSynchronize(b.ctx->stream2); }

    // the mask of a phase: the chunks `in` names, every other chunk inactive in it
    template <class In> void mask(In in) { for (size_t f = 0; f < n; f++) b.active[f] = in(jobs[f]) ? 1 : 0; }
    // the phases, in the reference's order
    int analyse(); void first_probe(); void search_1(); void queue_search_2(); bool residual_layer(); void truncation_search();
    bool entropy_and_fallback(); int assemble(uint8_t **outs, size_t *sizes);
    void start_search_2();
    void rate_search(int k, int lane = 0, int part = kSearchAll);
};

// Rate search k (0: error-bounded :728, 1: pure base layer :836) of every chunk with its state machine on the device
// (search.hpp): the rounds are enqueued back to back - advance, rate allocation, probe decode - without a host
// synchronisation in between; the host looks at the states once after `rounds` of them (EBCC_HIP_SEARCH_ROUNDS, default
// 16: more than the usual search needs) and only enqueues more if a chunk is still searching.
// lane 1: the search runs on the engine's second stream with its own state, counters and active mask, beside whatever
// the first stream does (search #2 beside the residual layer).  part: enqueue the first batch of rounds only
// (kSearchStart: no host synchronisation), or take the search up from there (kSearchFinish), or both.
void BatchEncode::rate_search(int k, int lane, int part)
{
    ebcc_hip_ctx *ctx = b.ctx;
    DevChunk *h = static_cast<DevChunk *>(ctx->h_search) + (size_t) lane * ctx->max_frames, *d = static_cast<DevChunk *>(ctx->d_search) + (size_t) lane * ctx->max_frames;
    int *const d_counter = ctx->d_counter + 4 * lane, *const h_counter = ctx->h_counter + 4 * lane;
    int *const d_active = lane ? ctx->d_active + ctx->max_frames : b.d_active;
    hipStream_t s = lane ? second_stream(ctx) : b.s;
    J2kBuffers &jb = b.jb;
    const int forced = getenv("EBCC_HIP_SPECULATION") ? atoi(getenv("EBCC_HIP_SPECULATION")) != 0 : -1;
    const bool speculate = lane == 0 && (forced >= 0 ? forced != 0 : slices <= 1);   // (lane 1 runs on the stream the candidates would use)
    hipStream_t s2 = nullptr;
    // probes that only steer the search stop counting once they are certainly infeasible (search.hpp); EBCC_HIP_NO_SHORTCUTS=1
    // and TRACE logging (which prints every probe's count) keep every probe exact
    double jobs_qt0 = 0.0;                                               // the error-bounded search's quantile target (0: it never ran)
    for (size_t f = 0; f < n; f++) if (jobs[f].search) { jobs_qt0 = jobs[f].rs[0].qt; break; }
    const double limit_qt = getenv("EBCC_HIP_NO_SHORTCUTS") || g_log_level <= 0 ? 0.0 : std::min(jobs_qt0, 1.0);
    auto advance = [&]() {
        launch_search_advance(d, jb.jf, d_active, (int) n, (int) b.tiles, k, (double) n_pix, d_counter, s,
                              speculate ? jb.cand_cr : nullptr, speculate ? jb.cand_sel : nullptr, limit_qt);
        if (speculate) launch_j2k_rate_publish(jb, (int) b.nt, s);
    };
    auto enqueue_rounds = [&](int rounds) {
        for (int r = 0; r < rounds; r++) {
            launch_j2k_rate(jb, (int) b.nt, d_active, s, speculate ? jb.have_rate : nullptr);
            if (speculate) {
                // the candidates read the record of bisection steps this k_rate may have extended, and the masks / rates of
                // the advance: after both; the next advance reads their results: after them
                EBCC_HIP_CHECK(hipEventRecord(ctx->ev_a, s));
                EBCC_HIP_CHECK(hipStreamWaitEvent(s2, ctx->ev_a, 0));
                launch_j2k_rate_candidates(jb, (int) b.nt, d_active, s2);
                EBCC_HIP_CHECK(hipEventRecord(ctx->ev_b, s2));
            }
            launch_j2k_probe_decode(b.d_frames, jb, (int) b.nt, d_active, s, k == 0 ? 2 : 0);     // (the field is stored where the advance asked for it: search.hip keeps_field)
            if (speculate) EBCC_HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_b, 0));
            advance();
        }
    };
    if (part != kSearchFinish) {
        for (size_t f = 0; f < n; f++) {
            const Job &j = jobs[f];
            DevChunk &c = h[f];
            c.const_field = j.const_field ? 1 : 0;
            c.state_cr = b.state_cr[f];
            c.q = j.q;
            c.n_probes = (int) std::min<size_t>(j.probes.size(), kMaxProbes);
            std::copy_n(j.probes.begin(), c.n_probes, c.probes);
            c.rs[k] = j.rs[k];
            if (!j.search) c.rs[k].phase = 6;                                  // (constant, or a mode without searches: never active)
        }
        EBCC_HIP_CHECK(hipMemcpyAsync(d, h, sizeof(DevChunk) * n, hipMemcpyHostToDevice, s));
        EBCC_HIP_CHECK(hipMemsetAsync(d_counter, 0, sizeof(int) * 4, s));
        // a round = the probe the previous advance asked for (rate allocation + decode of the active chunks), then the advance
        // that takes it in and asks for the next one.  Speculative rate allocation: a
        // step of the search can go two ways, so the layers of both rates it may ask for next are worked out on the engine's
        // second stream while the first stream decodes the current probe; the advance then takes the matching one over
        // (k_rate_publish) and the round's own k_rate only runs for the frames whose rate was not among the guesses.
        // It shortens a slice's chain (search #1 of 256 frames in one slice: 33 -> 29 ms) at the price of two more k_rate per
        // round; with several slices in flight the chip has no idle issue slots left to pay with (four slices: encode 7.7 GB/s
        // without, 6.7 with) - so it is on for a batch that runs as one slice, off otherwise; EBCC_HIP_SPECULATION=1 / 0 forces it.
        if (speculate) {
            s2 = second_stream(ctx);
            if (!ctx->ev_a) {
                EBCC_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_a, hipEventDisableTiming));
                EBCC_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_b, hipEventDisableTiming));
            }
            EBCC_HIP_CHECK(hipMemsetAsync(jb.cand_cr, 0xFF, sizeof(float) * 2 * b.nt, s));       // (NaN: no candidate matches)
            EBCC_HIP_CHECK(hipMemsetAsync(jb.have_rate, 0, sizeof(int) * b.nt, s));
        }
        advance();
        enqueue_rounds(search_rounds());
    }
    if (part == kSearchStart) return;
    if (speculate && !s2) s2 = second_stream(ctx);
    for (;;) {
        EBCC_HIP_CHECK(hipMemcpyAsync(h, d, sizeof(DevChunk) * n, hipMemcpyDeviceToHost, s));
        EBCC_HIP_CHECK(hipMemcpyAsync(h_counter, d_counter, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
        wait_stream(s);
        bool done = true;
        for (size_t f = 0; f < n; f++) done &= h[f].rs[k].phase == 6;
        if (done) break;
        enqueue_rounds(6);
    }
    log_trace("rate search %d: %d probes of chunks over the rounds", k, h_counter[0]);
    if (getenv("EBCC_HIP_PHASE_TIMING")) {
        int most = 0; long long sum = 0;
        for (size_t f = 0; f < n; f++) { most = std::max(most, h[f].n_probes); sum += h[f].n_probes; }
        fprintf(stderr, "ebcc-mi355x rate search %d: %d probes over the rounds, probes on record per chunk: mean %.1f, most %d\n", k, h_counter[0], (double) sum / (double) n, most);
    }
    if (getenv("EBCC_HIP_T1_STATS") && slices <= 1) j2k_probe_hist_dump(k == 0 ? "search #1" : "search #2");
    for (size_t f = 0; f < n; f++) {
        Job &j = jobs[f];
        if (!j.search) continue;
        const DevChunk &c = h[f];
        j.rs[k] = c.rs[k];
        if (k == 0) j.q = c.q;
        j.probes.assign(c.probes, c.probes + c.n_probes);
        b.state_cr[f] = c.state_cr;
    }
    b.fetch_jf(s);                                                        // (the host mirror of the per-frame scalars follows the device again)
}


// ---- :671-692: statistics, scaling, transform, tier-1 - once per frame.  NaN / Inf and a range that overflows float
//      refuse the batch (2, 1); 0: the chunks are analysed, their jobs hold min / max / target
int BatchEncode::analyse()
{
    ebcc_hip_ctx *ctx = b.ctx, *rc = b.rc;
    const size_t tiles = b.tiles, nt = b.nt;
    launch_input_stats(b.d_frames, (int) nt, ctx->n_pix, ctx->rb.fs, b.s);
    if (tiles > 1) combine_chunk_states(ctx, n, tiles);
    launch_j2k_analysis(b.d_frames, b.jb, (int) nt, b.s);
    next.release();                                                    // the next slice may start: this one's first stage is queued
    fetch_frame_states(ctx, nt);
    b.fetch_jf();
    if (j2k_tier1_retry(b.jb, (int) nt, b.tjf, b.s)) b.fetch_jf();    // (a group's decisions outgrew the segmented encoder's buffer)
    for (size_t f = 0; f < n; f++) {
        const FrameState &t0 = ctx->h_fs[f * tiles];                   // (all tiles of a chunk carry the chunk's statistics)
        if (t0.has_nonfinite) { log_fatal("NaN or Inf found in data of frame %zu", f); return 2; }
        if (b.jf[f].overflow) { log_fatal("code-block byte slot overflow in frame %zu", f); return 1; }
        if (jobs[f].fc.searching() && !t0.const_field && !std::isfinite(t0.maxv - t0.minv)) {
            // max - min overflows: the decoded base layer is (s / 65535) * inf + min (:1130), every residual is NaN or
            // infinite, and the reference stops on assert(dc0 >= 0 && dc0 <= MAXELEM) in spiht_encode (spiht_re.c:462)
            log_fatal("range of frame %zu overflows float (max - min = inf)", f);
            set_error("frame %zu: max - min overflows float", f);
            return 1;
        }
        jobs[f].const_field = t0.const_field != 0;
        jobs[f].minv = t0.minv;
        jobs[f].maxv = t0.maxv;
        jobs[f].search = !jobs[f].const_field && jobs[f].fc.searching();
        any_search |= jobs[f].search;
        b.jf[f].cr = jobs[f].fc.base_cr;
        b.jf[f].target = 0;
        b.active[f] = jobs[f].const_field ? 0 : 1;
    }
    if (rc != ctx) {                                                   // chunk-level frame states of the residual engine
        for (size_t f = 0; f < n; f++) {
            FrameState &r = rc->h_fs[f];
            r = FrameState{};
            r.minv = jobs[f].minv; r.maxv = jobs[f].maxv; r.const_field = jobs[f].const_field;
        }
        push_frame_states(rc, n);
    }
    pt.mark("analysis (dwt, tier-1, ckpt)");
    return 0;
}

// ---- :693-716: the first encode at base_cr and, unless NONE, its decode (:707-709) and the residual range of that decode
void BatchEncode::first_probe()
{
    ebcc_hip_ctx *rc = b.rc;
    // the chunks whose first encode is decoded: every mode but NONE.  A chunk in mode NONE takes the allocation alone.
    auto decoded = [](const Job &j) { return !j.const_field && j.fc.mode != NONE; };
    const bool any_none = std::any_of(jobs.begin(), jobs.end(), [](const Job &j) { return !j.const_field && j.fc.mode == NONE; });
    const bool need_decode = std::any_of(jobs.begin(), jobs.end(), [](const Job &j) { return j.fc.mode != NONE; });
    for (size_t f = 0; f < n; f++) {
        if (jobs[f].fc.mode == NONE) continue;
        float target = jobs[f].fc.error;                                                      // :723-726
        if (jobs[f].fc.mode == RELATIVE_ERROR) target *= jobs[f].maxv - jobs[f].minv;
        jobs[f].target = target;
        b.jf[f].target = target;
    }
    b.allocate();
    if (need_decode) {
        // (the allocation's mask is still on its way out of the pinned mirror: it must have left before the mirror changes)
        if (any_none) { wait_stream(b.s); mask(decoded); b.push_active(); }
        launch_j2k_probe_decode(b.d_frames, b.jb, (int) b.nt, b.d_active, b.s);
    }
    b.fetch_jf();
    if (need_decode) {
        for (size_t f = 0; f < n; f++) {
            if (!decoded(jobs[f])) continue;
            jobs[f].mean_err = b.jf[f].err_sum / (double) n_pix;                              // :709
            jobs[f].q = jobs[f].q_first = 1. - ((double) b.jf[f].nbad / (double) n_pix);
            jobs[f].cr = jobs[f].fc.base_cr;
            jobs[f].probes.push_back(DevProbe{b.jf[f].cr, b.jf[f].stream_bytes, b.jf[f].nbad, b.jf[f].err_sum, 1, 0});
            b.state_cr[f] = b.jf[f].cr;
        }
        // residual range of the first decode: only the header fields survive when no search runs (:716)
        launch_residual_minmax(b.d_frames, b.jb.DEC, (int) n, n_pix, rc->rb.fs, b.rs);
        fetch_frame_states(rc, n);
        for (size_t f = 0; f < n; f++)
            if (jobs[f].fc.mode != NONE) { jobs[f].rmin = rc->h_fs[f].rmin; jobs[f].rmax = rc->h_fs[f].rmax; }
    }
    // the chunks that are done with this encode: mode NONE, and stale enum values, which fall through to a base-only
    // stream behind their decode (quirk Q2)
    if (std::any_of(jobs.begin(), jobs.end(), [](const Job &j) { return !j.const_field && !j.search; })) {
        mask([](const Job &j) { return !j.const_field && !j.search; });
        b.collect_tails(jobs);
    }
    pt.mark("first probe");
}

// ---- :728: rate search #1 (error-bounded) and the codestreams of its result
void BatchEncode::search_1()
{
    for (size_t f = 0; f < n; f++)
        if (jobs[f].search) jobs[f].rs[0] = rate_search_start(jobs[f].fc.base_cr, jobs[f].q, q_target);
    rate_search(0);
    for (size_t f = 0; f < n; f++) {
        b.active[f] = jobs[f].search ? 1 : 0;
        if (jobs[f].search) { jobs[f].cr = jobs[f].rs[0].result; jobs[f].len1 = (size_t) jobs[f].rs[0].last.stream_bytes; }
    }
    pt.mark("rate search 1");
    // base layer of search #1.  (Sending the codestreams off without waiting for them - written and packed on the second
    // search's stream, fetched at the assembly - was measured: the slice's next stages are queued 2 ms earlier and the step
    // gets 1 - 5 ms LONGER, three alternating runs on two boxes; the wait stays.)
    b.collect_tails(jobs);
}

// :829-833: search #2 restarts from base_cr with the quantile of the first probe (== a re-encode at base_cr), or - that
// consistency step disabled - from search #1's state
void BatchEncode::start_search_2()
{
    for (Job &j : jobs)
        if (j.search) j.rs[1] = env.no_consistency ? rate_search_start(j.cr, j.q, 1.0) : rate_search_start(j.fc.base_cr, j.q_first, 1.0);
}

// ---- the pure base-layer search (:819-836) depends on nothing the residual layer produces: for one-frame chunks its rounds
//      are queued on the engine's second stream now (own state, counters and mask: rate_search lane 1) and run beside the
//      residual layer and the truncation search; it is taken up again where the reference runs it (entropy_and_fallback).
//      Round 2 measured this slower - the search was hidden behind the level-22 zstd of every prefix then; with the entropy
//      stage cut down to the prefixes whose size can matter, the search was what the slice waited for, and its sizes are
//      what decides which prefixes those are.
void BatchEncode::queue_search_2()
{
    if (!overlap2) return;
    start_search_2();
    rate_search(1, 1, kSearchStart);
    search2_queued = true;
}

// ---- :730-762: the residual range of search #1's decode, then for the chunks it does not leave within the target SPIHT
//      with a budget of the base layer's size, the probe of the whole stream, and "could not reach the target"
bool BatchEncode::residual_layer()
{
    ebcc_hip_ctx *rc = b.rc;
    hipStream_t rs = b.rs;
    launch_residual_minmax(b.d_frames, b.jb.DEC, (int) n, n_pix, rc->rb.fs, rs);          // :730-733
    fetch_frame_states(rc, n);
    for (size_t f = 0; f < n; f++) {
        Job &j = jobs[f];
        b.active[f] = 0;
        if (!j.search) continue;
        j.rmin = rc->h_fs[f].rmin; j.rmax = rc->h_fs[f].rmax;
        float cur = fmaxf(fabsf(j.rmin), fabsf(j.rmax));                                  // :735
        j.skip = cur <= j.target;                                                         // :737
        if (!j.skip) { b.active[f] = 1; any_resid = true; }
    }
    pt.mark("tails + residual range");
    if (!zstd().ok) { log_fatal("libzstd not available"); return false; }
    if (!any_resid) return true;
    // :744-754 (budgets, the encoder, the cut "everything" and its probe are queued without a look at the frame states in
    // between: the budget follows from the base layer's size, the whole stream's length stays on the device)
    b.push_ractive();
    launch_pad_and_dc(b.d_frames, b.jb.DEC, rc->rb, (int) n, rc->d_active, rs);
    launch_analysis(rc->rb, (int) n, rc->d_active, rs);
    for (size_t f = 0; f < n; f++) rc->h_u64a[f] = (unsigned long long) jobs[f].len1 * 8 + 128;   // bits0 = trunc_bits + 128
    EBCC_HIP_CHECK(hipMemcpyAsync(rc->d_u64a, rc->h_u64a, n * sizeof(unsigned long long), hipMemcpyHostToDevice, rs));
    launch_residual_budget(rc->rb, (int) n, rc->d_u64a, rc->d_active, rs);
    launch_spiht_encode(rc->rb, (int) n, rc->d_u64a, rc->d_active, rs);
    launch_whole_stream_cut(rc->rb, (int) n, rc->d_u64b, rc->d_active, rs);
    launch_prefix_synthesis_stats(b.d_frames, b.jb.DEC, rc->rb, (int) n, rc->d_u64b, rc->d_active, rs);   // full decode, :749
    fetch_frame_states(rc, n);
    pt.mark("residual: analysis, SPIHT, whole-stream probe");
    for (size_t f = 0; f < n; f++) {
        Job &j = jobs[f];
        if (!b.active[f]) continue;
        j.coeffs_orig = j.coeffs_size = rc->h_fs[f].stream_bytes;
        float cur = u2f(rc->h_fs[f].maxerr_bits);                                        // :754
        if (cur > j.target) {                                                             // :755-759
            log_info("frame %zu: could not reach error target %f (%f instead); retry with pure base compression", f, j.target, cur);
            j.skip = true; j.need_pure = true;
        } else {
            j.best_err = cur;
            j.mean_err = rc->h_fs[f].err_sum / (double) n_pix;                           // :762
            j.t_hi = (double) j.coeffs_size * 8; j.t_lo = 112.0; j.t_best = j.t_hi;       // :766-776
            j.trunc_active = true;
        }
    }
    return true;
}

// ---- :765-796: truncation bisection of the SPIHT streams as the device state machine (search.hpp): advance, reconstruct the
//      decoder state at the cut, synthesis + statistics - enqueued back to back, one look at the states after a batch of
//      rounds, more rounds only while a chunk is still searching
void BatchEncode::truncation_search()
{
    ebcc_hip_ctx *rc = b.rc;
    hipStream_t rs = b.rs;
    if (any_resid) {
        DevChunk *h = static_cast<DevChunk *>(rc->h_search), *d = static_cast<DevChunk *>(rc->d_search);
        for (size_t f = 0; f < n; f++) {
            const Job &j = jobs[f];
            DevChunk &c = h[f];
            c.t_hi = j.t_hi; c.t_lo = j.t_lo; c.t_best = j.t_best; c.mean_err = j.mean_err; c.best_err = j.best_err;
            c.target = j.target; c.trunc_active = j.trunc_active ? 1 : 0; c.trunc_pending = 0;
        }
        EBCC_HIP_CHECK(hipMemcpyAsync(d, h, sizeof(DevChunk) * n, hipMemcpyHostToDevice, rs));
        EBCC_HIP_CHECK(hipMemsetAsync(rc->d_counter, 0, sizeof(int) * 4, rs));
        // rounds a chunk can still need: a cut halves the interval (rounded up to a byte: + 8 bits at most) until it is
        // 32 bits wide (:777), then one more advance sees that nothing is left
        auto rounds_left = [](const DevChunk &c) {
            if (!c.trunc_active) return 0;
            double w = c.t_hi - c.t_lo;
            int r = 1;
            while (w > 32 && r < 64) { w = w / 2 + 8; r++; }
            return r;
        };
        int cuts_left = 1;                                               // cuts the longest search still visits, + the advance that ends it
        for (size_t f = 0; f < n; f++) cuts_left = std::max(cuts_left, rounds_left(h[f]));
        const bool forced_rounds = getenv("EBCC_HIP_SEARCH_ROUNDS") != nullptr;
        // `rounds` rounds back to back, a look at the states, then `more` rounds at a time until no chunk is searching
        auto drive = [&](int rounds, int more, auto round) {
            for (;; rounds = more) {
                for (int r = 0; r < rounds; r++) round();
                EBCC_HIP_CHECK(hipMemcpyAsync(h, d, sizeof(DevChunk) * n, hipMemcpyDeviceToHost, rs));
                wait_stream(rs);
                if (std::none_of(h, h + n, [](const DevChunk &c) { return c.trunc_active != 0; })) return;
            }
        };
        // Look-ahead (search.hpp: launch_trunc_advance_multi): a round probes the cut :779 chooses now and the cuts either
        // outcome leads to - `levels` levels of the bisection tree, 2^levels - 1 cut slots per frame - so the search takes
        // 1 / levels of the rounds.  The rounds are latency (a chain of six small launches beside the other slices' work),
        // the probes off the path mostly stop early (a cut shorter than an infeasible one is infeasible too: its first wave
        // over the target ends it).  EBCC_HIP_TRUNC_LEVELS=1, or no room for the cut slots: one cut per round.
        int levels = getenv("EBCC_HIP_TRUNC_LEVELS") ? std::min(3, std::max(1, atoi(getenv("EBCC_HIP_TRUNC_LEVELS")))) : 2;
        while (levels > 1 && !ensure_cut_slots(rc, (int) n * ((1 << levels) - 1))) levels--;
        if (levels > 1) {
            const CutSlots &cs = rc->cut;
            const int n_slots = (int) n * ((1 << levels) - 1);
            auto advance = [&] { launch_trunc_advance_multi(d, rc->rb.fs, cs, (int) n, (double) n_pix, levels, rc->d_counter, rs); };
            advance();
            drive(forced_rounds ? search_rounds() : (cuts_left + levels - 1) / levels + 1, 3, [&] {
                launch_prefix_synthesis_slots(b.d_frames, b.jb.DEC, rc->rb, cs, n_slots, rs);
                advance();
            });
        } else {
            auto advance = [&] { launch_trunc_advance(d, rc->rb.fs, rc->d_u64b, rc->d_active, (int) n, (double) n_pix, rc->d_counter, rs); };
            advance();
            drive(forced_rounds ? search_rounds() : cuts_left + 1, 6, [&] {
                launch_prefix_synthesis_stats(b.d_frames, b.jb.DEC, rc->rb, (int) n, rc->d_u64b, rc->d_active, rs);
                advance();
            });
        }
        for (size_t f = 0; f < n; f++) {
            Job &j = jobs[f];
            const DevChunk &c = h[f];
            if (j.trunc_active) { j.t_hi = c.t_hi; j.t_lo = c.t_lo; j.t_best = c.t_best; j.mean_err = c.mean_err; j.best_err = c.best_err; }
            j.trunc_active = false;
        }
    }
    for (Job &j : jobs) {
        if (!j.search || j.skip) j.coeffs_size = j.need_pure ? j.coeffs_orig : 0;
        else j.coeffs_size = (size_t) (j.t_best / 8.);                                    // :796
    }
    pt.mark("truncation search");
}

// ---- :811-854: entropy stage of the kept SPIHT prefix on host cores (:811-817) and the pure base-layer fallback (:819-854).
//      Level-22 zstd is by far the longest host step (~160 ns per byte on one core: 1.3 core-seconds per 256 frames
//      of the bench workload on a box whose container has 16 CPUs), and the reference throws most of it away: the
//      compressed size z is compared with what the pure base-layer search gives (:838: len2 < z + len1), and for
//      ~95 % of ERA5-like frames the base layer alone wins.  So z is only worked out where it can matter: a frame
//      whose z is PROVABLY above len2 - len1 (zstd_size_lower_bound: the literals no match can cover cost at least
//      their entropy) takes the pure base layer without being compressed - the same decision, bytes unchanged.
bool BatchEncode::entropy_and_fallback()
{
    ebcc_hip_ctx *rc = b.rc;
    Entropy es(jobs, slices, env.zstd_level, pt.on);
    // the kept SPIHT prefixes of the batch in one packed download; the workers read them where they land (the staging
    // buffer of the residual engine is not touched again before they are done)
    std::vector<size_t> coeff_len(n, 0), coeff_off(n, 0);
    for (size_t f = 0; f < n; f++) {
        if (jobs[f].coeffs_size <= 16) jobs[f].coeffs_size = 0;
        coeff_len[f] = jobs[f].coeffs_size;
    }
    stage_download(rc, (const uint8_t *) rc->rb.stream, rc->rb.stream_words * sizeof(uint32_t), coeff_len.data(), coeff_off.data(), n, b.rs);
    std::vector<size_t> with_prefix;
    for (size_t f = 0; f < n; f++)
        if (coeff_len[f]) { es.coeff_ptr[f] = rc->h_stage + coeff_off[f]; with_prefix.push_back(f); }
    std::vector<size_t> cand;                                       // frames whose floor may decide them (search #2's sizes)
    if (!want_pure) {
        es.submit_zstd(es.longest_first(with_prefix));                  // no fallback: every prefix is part of its stream
    } else {
        // frames whose residual layer could not reach the target are coded by the base layer whatever z is (:838 need_pure)
        const bool use_floor = zstd_floor_usable() && !getenv("EBCC_HIP_NO_SHORTCUTS");
        std::vector<size_t> now;
        for (size_t f : with_prefix) {
            if (jobs[f].need_pure) { es.zstate[f] = Entropy::kSkipped; continue; }
            (use_floor && jobs[f].coeffs_size <= kZstdFloorMaxBytes ? cand : now).push_back(f);
        }
        if (!now.empty()) es.submit_zstd(es.longest_first(now));
        if (!cand.empty()) es.submit_floors(cand);
    }
    pt.mark("zstd: queued");
    if (want_pure) {
        // search #2 re-uses every probe search #1 made; it runs while host cores work on the prefixes: first the floors (a
        // few microseconds per KB), then - the search still running on the GPU, len2 not known yet - zstd of the candidates
        // in the order in which they are likely to need it; the moment the search's sizes are in, the candidates they
        // decide are struck from the queue
        if (overlap2) {
            // the search has been running beside the residual layer: its sizes are (nearly) there, the floors take a
            // millisecond - the prefixes that are still open after that are compressed, longest first
            rate_search(1, 1, kSearchFinish);                                                 // :836
            search2_queued = false;
            pt.mark("rate search 2");
            gpu_phase_over.tell();                                                            // (what follows is host work and one small launch)
            if (!es.join_floors()) return false;
        } else {
            start_search_2();
            rate_search(1, 0, kSearchStart);
            if (!cand.empty()) {
                if (!es.join_floors()) return false;
                es.submit_zstd(es.lowest_floor_first(cand));
            }
            rate_search(1, 0, kSearchFinish);                                                 // :836
            pt.mark("rate search 2");
            gpu_phase_over.tell();
        }
        long long skipped_bytes = 0, skipped = 0;
        for (size_t f : cand)
            if (es.floor_decides(f) && es.strike(f)) { skipped++; skipped_bytes += (long long) jobs[f].coeffs_size; }
        if (overlap2) {
            const std::vector<size_t> open = es.not_started(cand);
            if (!open.empty()) es.submit_zstd(es.longest_first(open));
        }
        if (!es.join_all()) return false;
        pt.mark("zstd: wait for the workers");
        for (size_t f : with_prefix) if (jobs[f].need_pure) { skipped++; skipped_bytes += (long long) jobs[f].coeffs_size; }
        es.report(with_prefix, skipped, skipped_bytes);
        // :838-854: the pure base layer where it beats base + residual, or where the residual layer could not reach the target
        bool any_pure = false;
        for (size_t f = 0; f < n; f++) {
            Job &j = jobs[f];
            b.active[f] = 0;
            if (!j.search) continue;
            const size_t len2 = (size_t) j.rs[1].last.stream_bytes;
            const bool decided = es.floor_decides(f);                                         // (z may not be known - only that it loses)
            if (decided || len2 < j.zbytes.size() + j.len1 || j.need_pure) {                  // :838
                if (decided) log_info("frame %zu: pure base compression (%zu) beats base (%zu) + residual (at least %zu)", f, len2, j.len1, es.zfloor[f]);
                else if (len2 < j.zbytes.size() + j.len1)
                    log_info("frame %zu: pure base compression (%zu) beats base (%zu) + residual (%zu)", f, len2, j.len1, j.zbytes.size());
                j.mean_err = j.rs[1].last.err_sum / (double) n_pix;                           // :843
                j.zbytes.clear(); j.coeffs_size = 0;
                b.active[f] = 1; b.jf[f].cr = j.rs[1].result; any_pure = true;
            }
        }
        if (any_pure) { b.allocate(); b.collect_tails(jobs); }           // (that rate's layer assignment again, no decode)
    }
    if (!es.join_all()) return false;
    host_stats().add(es.zstd_us.load() + es.bound_us.load(), es.wait_us, es.zstd_bytes.load());
    return true;
}

// ---- :863-907: the frame streams - header, zstd payload, codestream (or the sample count of a constant field)
int BatchEncode::assemble(uint8_t **outs, size_t *sizes)
{
    for (size_t f = 0; f < n; f++) {
        Job &j = jobs[f];
        float minv = j.minv, maxv = j.maxv;
        log_info("frame %zu: mean of compression error %e", f, j.mean_err);
        if (!env.no_mean_adjust && std::fabs(j.mean_err) > 1e-18) {
            minv += j.mean_err;
            maxv += j.mean_err;
        }
        const size_t codec_size = j.const_field ? sizeof(uint64_t) : j.tail.size();
        const size_t total = sizeof(FrameHeader) + j.zbytes.size() + codec_size;
        uint8_t *o = (uint8_t *) malloc(total), *p = o;
        if (!o) { log_fatal("out of memory"); return 1; }
        FrameHeader hd;
        memset(&hd, 0, sizeof hd);
        memcpy(hd.magic, EBCC_HEADER_MAGIC, 4);
        hd.version = EBCC_HEADER_VERSION;
        if (j.const_field) hd.flags |= EBCC_HEADER_FLAG_CONST_FIELD;
        hd.minval_bits = f2u(minv); hd.maxval_bits = f2u(maxv);
        hd.coeffs_size = j.coeffs_size;
        hd.rmin_bits = f2u(j.const_field ? 0.0f : j.rmin); hd.rmax_bits = f2u(j.const_field ? 0.0f : j.rmax);
        hd.compressed_size = j.zbytes.size(); hd.tail_size = codec_size;
        memcpy(p, &hd, sizeof hd); p += sizeof hd;
        if (!j.zbytes.empty()) { memcpy(p, j.zbytes.data(), j.zbytes.size()); p += j.zbytes.size(); }
        if (j.const_field) { uint64_t cnt = n_pix; memcpy(p, &cnt, 8); }
        else memcpy(p, j.tail.data(), j.tail.size());
        log_info("frame %zu: coeffs_size %zu compressed_size %zu jp2_length %zu ratio %f", f, j.coeffs_size, j.zbytes.size(),
                 codec_size, (double) (n_pix * 4) / (double) total);
        outs[f] = o;
        sizes[f] = total;
    }
    pt.mark("assemble");
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// ebcc_encode for a batch of device-resident single-frame chunks.  Returns 0, 1 (error) or 2 (NaN/Inf).
// ------------------------------------------------------------------------------------------------
// `n` chunks of `tiles` frames each (tiles == 1: the frame-per-chunk case); `rctx`: residual engine for the stacked
// chunk image when tiles > 1.
int encode_batch(ebcc_hip_ctx *ctx, const float *d_frames, size_t n, const FrameConfig *fc, uint8_t **outs, size_t *sizes,
                 SliceGate *next, size_t tiles, ebcc_hip_ctx *rctx, unsigned slices, PhaseNote *note)
{
    BatchEncode e(ctx, d_frames, n, fc, next, tiles, rctx, slices, note);
    if (const int r = e.analyse()) return r;                          // :671-692 (releases `next`)
    e.first_probe();                                                  // :693-716
    if (e.any_search) {
        e.search_1();                                                 // :728
        e.queue_search_2();                                           // (:836, beside what follows)
        if (!e.residual_layer()) return 1;                            // :730-762
        e.truncation_search();                                        // :765-796
        if (!e.entropy_and_fallback()) return 1;                      // :811-854 (tells `note`)
    }
    e.pt.mark("fallback search + tails");
    return e.assemble(outs, sizes);                                   // :863-907
}


// One frame stream, either format: the 48-byte "EBCC" header (:190-202, :1234-1260) or the legacy header-less
// prefix `f32 min, f32 max, u64 coeffs_size, f32 rmin, f32 rmax, u64 compressed_size` (ebcc_decode_legacy,
// :1147-1213), where a constant field is signalled by min == max.
bool parse_frame(const uint8_t *d, size_t len, ParsedFrame &pf)
{
    if (len >= sizeof(FrameHeader) && memcmp(d, EBCC_HEADER_MAGIC, 4) == 0) {
        FrameHeader hd;
        memcpy(&hd, d, sizeof hd);
        if (hd.version != EBCC_HEADER_VERSION) { log_fatal("Unsupported EBCC header version: %u", hd.version); return false; }
        size_t used = sizeof hd;
        if (hd.compressed_size > len - used) { log_fatal("Invalid encoded data: truncated payload"); return false; }   // :1249
        used += hd.compressed_size;
        if (hd.tail_size > len - used) { log_fatal("Invalid encoded data: truncated payload"); return false; }         // :1254
        used += hd.tail_size;
        if (used != len) { log_fatal("Invalid encoded data: payload size mismatch"); return false; }                  // :1314
        pf.minv = u2f(hd.minval_bits); pf.maxv = u2f(hd.maxval_bits);
        pf.rmin = u2f(hd.rmin_bits); pf.rmax = u2f(hd.rmax_bits);
        pf.const_field = (hd.flags & EBCC_HEADER_FLAG_CONST_FIELD) != 0;
        pf.coeffs_size = hd.coeffs_size; pf.compressed_size = hd.compressed_size; pf.tail_size = hd.tail_size;
        pf.z = d + sizeof hd; pf.tail = pf.z + hd.compressed_size;
        if (pf.const_field && hd.tail_size != sizeof(uint64_t)) {
            log_fatal("Invalid encoded data: const-field payload must contain uint64_t length");
            return false;
        }
    } else {
        const size_t prefix = 4 + 4 + 8 + 4 + 4 + 8;
        if (len < prefix) { log_fatal("Invalid legacy encoded data: truncated header"); return false; }
        uint64_t cs, zs;
        memcpy(&pf.minv, d, 4); memcpy(&pf.maxv, d + 4, 4); memcpy(&cs, d + 8, 8);
        memcpy(&pf.rmin, d + 16, 4); memcpy(&pf.rmax, d + 20, 4); memcpy(&zs, d + 24, 8);
        if (zs > len - prefix) { log_fatal("Invalid legacy encoded data: truncated residual payload"); return false; }
        pf.coeffs_size = cs; pf.compressed_size = zs;
        pf.z = d + prefix; pf.tail = pf.z + zs; pf.tail_size = len - prefix - zs;
        pf.const_field = pf.minv == pf.maxv;
        if (pf.const_field && pf.tail_size < sizeof(uint64_t)) { log_fatal("Invalid legacy encoded data: missing const-field length"); return false; }
    }
    if (pf.const_field && pf.compressed_size > 0 && pf.coeffs_size > 0) {
        log_fatal("Invalid encoded data: residual data cannot be applied to const field");
        return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// ebcc_decode for a batch of chunk streams -> device buffer d_out [n][chunk pixels]
// ------------------------------------------------------------------------------------------------
// The chunks of encode_batch: chunk c is the frames c * tiles .. c * tiles + tiles - 1 of `ctx` - for tiles > 1 the
// tile-parts of one tiled codestream (reference :121-125) - and its residual layer one frame of `rctx` (== ctx for
// one-frame chunks).
int decode_batch(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n, float *d_out,
                 SliceGate *next, size_t tiles, ebcc_hip_ctx *rctx, const DecodeRegion &region)
{
    struct Release { SliceGate *g; ~Release() { if (g) g->release(); } } release_on_exit{next};
    ebcc_hip_ctx *const rc = rctx ? rctx : ctx;
    J2kBuffers &jb = *static_cast<J2kBuffers *>(ctx->j2k);
    hipStream_t s = ctx->stream;
    const size_t nt = n * tiles, n_pix = ctx->n_pix * tiles;         // frames of ctx; pixels of a chunk
    const J2kGeom &g = jb.geom;
    // The plan of the region, made (or refused) before anything is written: what the kernels put out (`dev`: the window's cone,
    // or the table of the boxes with the spans of their cones) and `keep`, whether a code-block holds any of it - one row for
    // every frame (keep_row 0: a window) or a row per frame (a box list: the union over the frame's boxes); empty: all do.
    J2kRegion dev;
    std::vector<uint8_t> keep;
    size_t keep_row = 0;
    if (region.kind != DecodeRegion::Frames) {
        const bool window = region.kind == DecodeRegion::Window;
        if (tiles != 1 || g.period != 1) { set_error("%s decode: chunks of several frames are not supported", window ? "window" : "box"); return 1; }
        dev.kind = window ? J2kRegion::Window : J2kRegion::List;
        dev.out = d_out;
        if (window) {
            if (!j2k_window_supported(g)) { set_error("window decode: frames of %d x %d are not supported (fewer than 3 columns)", g.H, g.W); return 1; }
            if (!j2k_window_plan(g, region.row0, region.col0, region.rows, region.cols, dev.cone)) {
                set_error("window decode: the window is empty or not inside the %d x %d frame", g.H, g.W);
                return 1;
            }
            std::vector<J2kBlock> blocks;
            make_j2k_geom(g.H, g.W, blocks);
            keep.resize(blocks.size());
            int rect[4];
            for (size_t b = 0; b < blocks.size(); b++) keep[b] = j2k_window_keeps(g, blocks[b], dev.cone, rect) ? 1 : 0;
        } else {
            std::vector<ebcc_hip_placed_box> local(region.list, region.list + region.n);
            for (ebcc_hip_placed_box &b : local) b.frame -= region.frame0;
            keep_row = (size_t) g.nblocks;
            keep.resize(n * keep_row);
            boxes_reserve(ctx, region.n, sizeof(J2kBoxEntry) + sizeof(J2kPlacement));
            J2kBoxEntry *const h_table = static_cast<J2kBoxEntry *>(ctx->boxes.h), *const table = static_cast<J2kBoxEntry *>(ctx->boxes.d);
            dev.list = J2kBoxList{h_table, table, reinterpret_cast<J2kPlacement *>(h_table + region.n), reinterpret_cast<J2kPlacement *>(table + region.n), region.n, 0, 0};
            if (!j2k_list_check("list decode", g, n, local.data(), local.size(), region.out_floats, keep.data(), h_table, dev.list.h_place, j2k_first_fused(jb),
                                &dev.list.rows, &dev.list.cols)) return 1;
        }
    }
    const size_t out_pix = region.pixels(n_pix);                      // samples of an output item
    int *const table = ctx->h_table;                                  // (pinned)
    const size_t table_ints = nt * (size_t) g.stride * 4;
    memset(table, 0, table_ints * sizeof(int));
    // pieces to upload: codestream (tiles == 1) or tile-part k of chunk c at c * tiles + k, found at src_off in the
    // chunk's tail; SPIHT bytes of chunk c at nt + c - staged in pinned memory and sent as one copy
    std::vector<size_t> piece(nt + n, 0), piece_off(nt + n, 0), src_off(nt, 0);
    std::vector<ParsedFrame> heads(n);
    PhaseTimer pt;
    // frame states: the device's for one-frame chunks, zeroed ones for tiles and chunks; the header's fields are set below
    if (tiles == 1) fetch_frame_states(ctx, n);
    else { std::fill_n(ctx->h_fs, nt, FrameState{}); std::fill_n(rc->h_fs, n, FrameState{}); }
    // the host side of a batch - frame headers, packet headers, zstd of the residual streams - is per chunk and runs on a
    // few host threads (decode is one slice: nothing else hides it); a chunk's failure fails the batch
    std::atomic<bool> failed{false}, resid{false};
    // (the reason a chunk was rejected is written on the worker's thread - set_error's text is per thread; the first one is
    //  carried over to the calling thread, where ebcc_hip_last_error is read)
    auto for_chunks = [&](auto body) {
        const unsigned width = (unsigned) std::min<size_t>({(size_t) 16, (size_t) entropy_threads(1), (n + 7) / 8});
        auto batch = HostPool::instance().submit(n, width, [&](size_t c) {
            if (failed.load(std::memory_order_relaxed)) return;
            clear_error();
            if (!body(c)) {
                failed = true;
                const char *why = ebcc_hip_last_error();
                throw std::runtime_error(why && *why ? why : "invalid encoded data");
            }
        });
        if (!batch->wait()) { failed = true; set_error("%s", batch->error.c_str()); }
    };
    for_chunks([&](size_t c) -> bool {
        rc->h_active[c] = 0;
        ParsedFrame &hd = heads[c];
        if (!parse_frame(streams[c], sizes[c], hd)) return false;
        // the chunk's range on every tile (ctx), and with the residual range on the chunk (rc: the same state for tiles == 1)
        for (size_t t = c * tiles; t < (c + 1) * tiles; t++) {
            FrameState &fs = ctx->h_fs[t];
            fs.minv = hd.minv; fs.maxv = hd.maxv; fs.const_field = hd.const_field ? 1 : 0;
        }
        FrameState &fs = rc->h_fs[c];
        fs.minv = hd.minv; fs.maxv = hd.maxv;
        fs.rmin = hd.rmin; fs.rmax = hd.rmax;
        fs.const_field = hd.const_field ? 1 : 0;
        if (fs.const_field) {
            uint64_t cnt = 0;
            memcpy(&cnt, hd.tail, 8);
            if (cnt != n_pix) { log_fatal("const-field length %llu does not match the %s", (unsigned long long) cnt, tiles > 1 ? "chunk" : "frame"); return false; }
            return true;
        }
        int *const rows = table + c * tiles * g.stride * 4;
        if (tiles == 1) {
            if (hd.tail_size > jb.stream_cap) { log_fatal("codestream larger than the device slot"); return false; }
            if (!j2k_parse_codestream(hd.tail, hd.tail_size, g, rows)) return false;
            const uint8_t *const kept = keep.data() + c * keep_row;    // (window / box decode) a zeroed entry is a code-block without data
            for (size_t b = 0; b < (keep.empty() ? (size_t) 0 : (size_t) g.nblocks); b++)
                if (!kept[b]) rows[4 * b] = rows[4 * b + 1] = rows[4 * b + 2] = rows[4 * b + 3] = 0;
            piece[c] = hd.tail_size;
        } else {
            if (!j2k_parse_tiled(hd.tail, hd.tail_size, jb, (int) tiles, rows, &src_off[c * tiles], &piece[c * tiles])) {
                log_fatal("Invalid encoded data: %s", ebcc_hip_last_error());
                return false;
            }
            for (size_t t = c * tiles; t < (c + 1) * tiles; t++)
                if (piece[t] > jb.stream_cap) { log_fatal("tile-part larger than the device slot"); return false; }
        }
        if (hd.compressed_size > 0 && hd.coeffs_size > 0) {                                                    // :1294-1304
            if (!zstd().ok) { log_fatal("libzstd not available"); return false; }
            if (hd.coeffs_size > rc->rb.stream_words * 4 - 64) { log_fatal("residual stream larger than the device slot"); return false; }
            piece[nt + c] = hd.coeffs_size;
            rc->h_active[c] = 1;
            resid = true;
        }
        return true;
    });
    if (failed) return 1;
    const bool any_resid = resid;
    stage_reserve(ctx, piece.data(), piece_off.data(), nt + n);
    for_chunks([&](size_t c) -> bool {
        const ParsedFrame &hd = heads[c];
        for (size_t t = c * tiles; t < (c + 1) * tiles; t++)
            if (piece[t]) memcpy(ctx->h_stage + piece_off[t], hd.tail + src_off[t], piece[t]);
        if (piece[nt + c]) {
            // the residual stream: exactly coeffs_size bytes (the staging buffer holds whatever an earlier call left),
            // a SPIHT header for the chunk's grid and a bit budget the decoder can work with (:1294-1304)
            uint8_t *const z = ctx->h_stage + piece_off[nt + c];
            const size_t got = zstd().decompress(z, hd.coeffs_size, hd.z, hd.compressed_size);
            if ((zstd().is_error && zstd().is_error(got)) || got != hd.coeffs_size) { log_fatal("Invalid encoded data: residual payload does not decompress to %zu bytes", hd.coeffs_size); return false; }
            if (check_ims_header(rc, z, hd.coeffs_size, hd.coeffs_size * 8)) { log_fatal("Invalid encoded data: %s", ebcc_hip_last_error()); return false; }
        }
        return true;
    });
    if (failed) return 1;
    stage_send(ctx, nt + n, s);
    stage_scatter(ctx, jb.stream, jb.stream_cap, 0, nt, s);
    pt.mark("decode: parse, zstd, uploads");
    push_frame_states(ctx, nt);
    // The residual layer (SPIHT decode + synthesis: one wave per chunk, latency-bound) does not depend on the
    // base layer until the final addition, so it runs on the engine's second stream beside the tier-1 decode.
    hipStream_t s2 = s;
    if (any_resid) {
        if (rc != ctx) push_frame_states(rc, n, s);                   // (on s: ordered before the event like the rest)
        s2 = second_stream(ctx);
        if (!ctx->ev_a) {
            EBCC_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_a, hipEventDisableTiming));
            EBCC_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_b, hipEventDisableTiming));
        }
        EBCC_HIP_CHECK(hipEventRecord(ctx->ev_a, s));                       // frame states and the staged pieces are on the device
        EBCC_HIP_CHECK(hipStreamWaitEvent(s2, ctx->ev_a, 0));
    }
    // the residual stream is fed first: its one-wave-per-chunk kernel has to find a wave slot on every CU, and once the
    // tier-1 decoder's ~10^4 workgroups (longest code-blocks first) hold the slots none frees up for milliseconds
    if (any_resid) {
        const size_t slot = rc->rb.stream_words * 4;
        for (size_t c = 0; c < n; c++) {
            rc->h_u64a[c] = piece[nt + c];
            rc->h_u64b[c] = piece[nt + c] * 8;
        }
        stage_scatter(ctx, (uint8_t *) rc->rb.stream, slot, nt, n, s2);
        EBCC_HIP_CHECK(hipMemcpyAsync(rc->d_u64a, rc->h_u64a, n * sizeof(unsigned long long), hipMemcpyHostToDevice, s2));
        EBCC_HIP_CHECK(hipMemcpyAsync(rc->d_u64b, rc->h_u64b, n * sizeof(unsigned long long), hipMemcpyHostToDevice, s2));
        EBCC_HIP_CHECK(hipMemcpyAsync(rc->d_active, rc->h_active, n * sizeof(int), hipMemcpyHostToDevice, s2));
        launch_spiht_decode((const uint8_t *) rc->rb.stream, slot, rc->d_u64a, rc->d_u64b, rc->rb, (int) n, rc->d_active, s2);
        launch_synthesis_head(rc->rb, (int) n, rc->d_active, s2);
        if (s2 != s) EBCC_HIP_CHECK(hipEventRecord(ctx->ev_b, s2));
    }
    EBCC_HIP_CHECK(hipMemcpyAsync(jb.dec_table, table, table_ints * sizeof(int), hipMemcpyHostToDevice, s));
    // the decoded field is written where the caller wants it ([n][tiles][tile pixels] == [n][chunk pixels]; the engine's own
    // field buffer and a 1 GB device-to-device copy per 256 frames only for an output that is not aligned the way the
    // engine's buffers are)
    const bool direct = region.direct(d_out);
    J2kBuffers view = jb;
    if (direct && dev.kind == J2kRegion::Frames) view.DEC = d_out;
    launch_j2k_decode(view, (int) nt, s, table, dev);
    if (next) { next->release(); release_on_exit.g = nullptr; }     // host parsing done, kernels queued
    if (any_resid) {
        if (s2 != s) EBCC_HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_b, 0));
        // last row pass: field += residual (of a window or a box: its rows alone)
        if (dev.kind == J2kRegion::List) launch_synthesis_tail_add_placed(d_out, rc->rb, dev.list.table, dev.list.place, dev.list.n, rc->d_active, s, dev.list.rows);
        else if (dev.kind == J2kRegion::Window) launch_synthesis_tail_add(d_out, rc->rb, (int) n, rc->d_active, s, dev.cone.row0, dev.cone.col0, dev.cone.rows, dev.cone.cols);
        else launch_synthesis_tail_add(view.DEC, rc->rb, (int) n, rc->d_active, s, 0, 0, rc->rb.g.size_y, rc->rb.g.size_x);
    }
    if (!direct) EBCC_HIP_CHECK(hipMemcpyAsync(d_out, jb.DEC, n * n_pix * sizeof(float), hipMemcpyDeviceToDevice, s));
    // constant chunks: fill on the host side of the copy (rare path) - one host image per constant chunk, kept until the one
    // wait below.  (a list: a pitched fill on the device, from the frame states and the tables that are there already)
    std::vector<std::vector<float>> fills;
    if (dev.kind == J2kRegion::List) {
        bool any_const = false;
        for (size_t e = 0; e < dev.list.n && !any_const; e++) any_const = rc->h_fs[dev.list.h_table[e].frame].const_field != 0;
        if (any_const) launch_j2k_fill_placed(jb, dev.list, d_out, s);
    } else {
        for (size_t c = 0; c < n; c++) {
            if (!rc->h_fs[c].const_field) continue;
            fills.emplace_back(out_pix, rc->h_fs[c].minv);
            EBCC_HIP_CHECK(hipMemcpyAsync(d_out + c * out_pix, fills.back().data(), out_pix * sizeof(float), hipMemcpyHostToDevice, s));
        }
    }
    wait_stream(s);
    pt.mark("decode: kernels");
    return 0;
}

// Frame heights a chunk of several frames can have: OpenJPEG cannot set up 6 resolutions on smaller tiles (the
// reference crashes on them), and the chunk image itself is bounded by the reference's 2047-row limit.
bool tile_height_supported(size_t h) { return h >= 32 && h <= 1023; }
// Heights for which every tile has the geometry of a tile at the origin (sub-band extents, parity and code-block
// partition repeat): the context then needs a single geometry for all tile positions.
bool tile_geometry_uniform(size_t h) { return h >= 32 && h <= 1024 && (h & (h - 1)) == 0; }

}  // namespace ebcc
