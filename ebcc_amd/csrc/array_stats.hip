// array_stats.hip - what the entry points of host_codec.hip compute on arrays that lie on the device, outside the frame codec:
// the chunk gather of the container encode, the range of an array (and of many), the per-frame error statistics of the audit
// and the hard-bound encode, the fold over time of the reduce decode, and the regional statistics of the area series - the
// kernels, their launchers and the checks of their arguments (array_stats.hpp).  None of them is in the timed encode or decode
// chain.  The comments that state an order rule are the specification the tests check.
#include <climits>
#include "array_stats.hpp"
#include "time_walk.hpp"

namespace ebcc {

// ChunkBox::gather for an array on the device (one-frame chunks): chunks [first, first + gridDim.y) -> [chunk][ch][cw] at dst.
// A destination row is one contiguous run, cut into slots of four floats; a thread takes slots i, i + step, .. of its chunk,
// four of them in flight.  A slot that lies inside the real width of a source row on a 16-byte boundary is one 16-byte load,
// any other four clamped 4-byte loads (the padding columns repeat the row's last real sample, the padding rows the last row);
// a slot of a destination row on a 16-byte boundary is one 16-byte store.  Which width is taken changes no value.
namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct GatherArgs {
    const float *src;
    float *dst;
    size_t H, W, cnt1, cnt2, first;
    unsigned ch, cw;
};
__global__ __launch_bounds__(256) void k_gather_chunks(GatherArgs a)
{
    const size_t cl = a.first + blockIdx.y;
    const size_t r0 = (cl / a.cnt2 % a.cnt1) * a.ch, c0 = (cl % a.cnt2) * a.cw, t = cl / a.cnt2 / a.cnt1;
    const unsigned w = (unsigned) min((size_t) a.cw, a.W - c0);                     // real columns of this chunk
    const unsigned spr = (a.cw + 3) / 4, slots = a.ch * spr, step = gridDim.x * 256;
    const float *plane = a.src + t * a.H * a.W + c0;
    float *out = a.dst + (size_t) blockIdx.y * a.ch * a.cw;
    for (unsigned i0 = blockIdx.x * 256 + threadIdx.x; i0 < slots; i0 += 4 * step) {
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned i = i0 + k * step;
            if (i < slots) {
                const unsigned y = i / spr, x = 4 * (i - y * spr);
                const float *row = plane + min(r0 + y, a.H - 1) * a.W;
                if (x + 4 <= w && ((uintptr_t) row & 15) == 0) v[k] = *reinterpret_cast<const f32x4 *>(row + x);
                else v[k] = f32x4{row[min(x, w - 1)], row[min(x + 1, w - 1)], row[min(x + 2, w - 1)], row[min(x + 3, w - 1)]};
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned i = i0 + k * step;
            if (i < slots) {
                const unsigned y = i / spr, x = 4 * (i - y * spr);
                float *row = out + (size_t) y * a.cw;
                if (x + 4 <= a.cw && ((uintptr_t) row & 15) == 0) *reinterpret_cast<f32x4 *>(row + x) = v[k];
                else {
                    row[x] = v[k].x;
                    if (x + 1 < a.cw) row[x + 1] = v[k].y;
                    if (x + 2 < a.cw) row[x + 2] = v[k].z;
                    if (x + 3 < a.cw) row[x + 3] = v[k].w;
                }
            }
        }
    }
}
}  // namespace
// chunks [first, first + count) of a [..][H][W] array in chunks of ch x cw, enqueued on s (cnt1 x cnt2 chunks a frame)
void launch_gather_chunks(const float *d_array, size_t H, size_t W, size_t ch, size_t cw, size_t first, size_t count, float *d_out, hipStream_t s)
{
    const size_t slots = ch * ((cw + 3) / 4);
    const unsigned bx = (unsigned) std::min<size_t>(std::max<size_t>(1, slots / (256 * 4)), 64);
    for (size_t lo = 0; lo < count; lo += 65535) {                  // (gridDim.y)
        const size_t k = std::min<size_t>(65535, count - lo);
        const GatherArgs a{d_array, d_out + lo * ch * cw, H, W, cdiv(H, ch), cdiv(W, cw), first + lo, (unsigned) ch, (unsigned) cw};
        hipLaunchKernelGGL(k_gather_chunks, dim3(bx, (unsigned) k), dim3(256), 0, s, a);
    }
    EBCC_HIP_LAUNCH_CHECK();
}

// Global minimum and maximum of the floats of an array as order keys (float_order_key: -0 is +0), and whether a NaN or an Inf
// is among them - for many arrays in one launch (the variables of a model step, each with a bound relative to its own range;
// one array is a group of one): blockIdx.y is the group, its pointer and length one uniform load from `table`,
// out[3 * group ..] = {min key, max key, flag}, set to {~0, 0, 0} before the launch.  A group begins at any 4-byte alignment:
// the floats in front of the first 16-byte boundary and behind the last whole 16 bytes go one by one, the rest 16 bytes per
// lane, two loads in flight (as k_in_minmax, j2k_analysis.hip); the waves reduce by shuffle and add one atomic each per word.
// Minimum, maximum and an OR do not depend on the order: the result is exact.  The grid's x extent is that of the longest
// group: a workgroup that lies beyond a shorter group's body leaves at once (workgroup 0 never does: it holds the lanes of
// head and tail) - the test is uniform over the workgroup and no barrier follows it.
namespace {
struct GroupSpan { const float *x; size_t n; };
__global__ __launch_bounds__(256) void k_group_ranges(const GroupSpan *__restrict__ table, unsigned *__restrict__ out)
{
    const GroupSpan g = table[blockIdx.y];
    const float *__restrict__ x = g.x;
    const size_t n = g.n;
    const size_t lead = (size_t) ((16 - ((uintptr_t) x & 15)) & 15) / 4, head = lead < n ? lead : n, n4 = (n - head) >> 2;
    if (blockIdx.x != 0 && (size_t) blockIdx.x * blockDim.x >= n4) return;
    unsigned kmin = ~0u, kmax = 0u;
    int bad = 0;
    auto take = [&](float v) {
        if (isnan(v) || isinf(v)) bad = 1;
        const unsigned k = float_order_key(v);
        kmin = min(kmin, k);
        kmax = max(kmax, k);
    };
    const size_t gid = (size_t) blockIdx.x * blockDim.x + threadIdx.x, step = (size_t) gridDim.x * blockDim.x;
    if (gid < head) take(x[gid]);
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(x + head);
    size_t i = gid;
    for (; i + step < n4; i += 2 * step) {
        const f32x4 p = x4[i], q = x4[i + step];
        take(p.x); take(p.y); take(p.z); take(p.w);
        take(q.x); take(q.y); take(q.z); take(q.w);
    }
    if (i < n4) { const f32x4 p = x4[i]; take(p.x); take(p.y); take(p.z); take(p.w); }
    if (head + 4 * n4 + gid < n) take(x[head + 4 * n4 + gid]);
    for (int d = 32; d >= 1; d >>= 1) {
        kmin = min(kmin, (unsigned) __shfl_xor((int) kmin, d));
        kmax = max(kmax, (unsigned) __shfl_xor((int) kmax, d));
        bad |= __shfl_xor(bad, d);
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned *o = out + 3 * (size_t) blockIdx.y;
        atomicMin(&o[0], kmin);
        atomicMax(&o[1], kmax);
        if (bad) atomicOr(&o[2], 1u);
    }
}
}  // namespace
// keys[3 * g ..] = {min key, max key, non-finite flag} of the device arrays ptrs[g][0 .. lens[g]) (lens > 0, 4-byte aligned):
// one upload of the table, one launch (per 65535 groups), one download and one wait.  Device current, the context the caller's
// alone; table and words lie in the context's small pinned / device table (boxes_reserve).
void group_range_keys(ebcc_hip_ctx *ctx, const float *const *ptrs, const size_t *lens, size_t n, unsigned *keys)
{
    constexpr size_t rec = sizeof(GroupSpan) + 3 * sizeof(unsigned);
    boxes_reserve(ctx, n, rec);
    GroupSpan *h_t = (GroupSpan *) ctx->boxes.h, *d_t = (GroupSpan *) ctx->boxes.d;
    unsigned *h_o = (unsigned *) (h_t + n), *d_o = (unsigned *) (d_t + n);
    size_t longest = 0;
    for (size_t g = 0; g < n; g++) {
        h_t[g] = GroupSpan{ptrs[g], lens[g]};
        h_o[3 * g] = ~0u; h_o[3 * g + 1] = 0; h_o[3 * g + 2] = 0;
        longest = std::max(longest, lens[g]);
    }
    EBCC_HIP_CHECK(hipMemcpyAsync(d_t, h_t, n * rec, hipMemcpyHostToDevice, ctx->stream));
    const unsigned blocks = (unsigned) std::min<size_t>(std::max<size_t>(1, longest / (256 * 8)), 2048);
    for (size_t lo = 0; lo < n; lo += 65535) {                      // (gridDim.y)
        const size_t k = std::min<size_t>(65535, n - lo);
        hipLaunchKernelGGL(k_group_ranges, dim3(blocks, (unsigned) k), dim3(256), 0, ctx->stream, d_t + lo, d_o + 3 * lo);
    }
    EBCC_HIP_LAUNCH_CHECK();
    EBCC_HIP_CHECK(hipMemcpyAsync(h_o, d_o, n * 3 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    wait_stream(ctx->stream);
    memcpy(keys, h_o, n * 3 * sizeof(unsigned));
}
float float_of_order_key(uint32_t k) { return u2f((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
// One array, as a group of one -> 0 and {min, max}, or 2: NaN / Inf among the n floats (mm untouched).
int array_range(ebcc_hip_ctx *ctx, const float *d_data, size_t n, float mm[2])
{
    unsigned keys[3];
    group_range_keys(ctx, &d_data, &n, 1, keys);
    if (keys[2]) return 2;
    mm[0] = float_of_order_key(keys[0]); mm[1] = float_of_order_key(keys[1]);
    return 0;
}
// The same for arrays in host memory, on the process-wide pool in pieces of a million floats.
void host_range_keys(const float *const *ptrs, const size_t *lens, size_t n, unsigned *keys)
{
    constexpr size_t kPiece = (size_t) 1 << 20;
    struct Piece { size_t g, lo, hi; unsigned kmin = ~0u, kmax = 0, bad = 0; };
    std::vector<Piece> pieces;
    for (size_t g = 0; g < n; g++)
        for (size_t lo = 0; lo < lens[g]; lo += kPiece) pieces.push_back(Piece{g, lo, std::min(lens[g], lo + kPiece)});
    auto batch = HostPool::instance().submit(pieces.size(), entropy_threads(1), [&](size_t i) {
        Piece &p = pieces[i];
        const float *x = ptrs[p.g];
        unsigned kmin = ~0u, kmax = 0, bad = 0;
        for (size_t k = p.lo; k < p.hi; k++) {
            bad |= (f2u(x[k]) & 0x7F800000u) == 0x7F800000u;
            const unsigned key = float_order_key(x[k]);
            kmin = std::min(kmin, key); kmax = std::max(kmax, key);
        }
        p.kmin = kmin; p.kmax = kmax; p.bad = bad;
    });
    if (!batch->wait()) throw HipFailure(batch->error.c_str());
    for (size_t g = 0; g < n; g++) { keys[3 * g] = ~0u; keys[3 * g + 1] = 0; keys[3 * g + 2] = 0; }
    for (const Piece &p : pieces) {
        keys[3 * p.g] = std::min(keys[3 * p.g], p.kmin); keys[3 * p.g + 1] = std::max(keys[3 * p.g + 1], p.kmax); keys[3 * p.g + 2] |= p.bad;
    }
}

// Per-frame error statistics of decoded frames d against their originals x, both [gridDim.y][n_pix] (include/ebcc_hip.h:
// ebcc_hip_frame_error): blockIdx.y is the frame, blockIdx.x one of the frame's pieces - as many as frame_error_pieces gives for
// the pixel count, whatever the batch.  A lane takes the quads (pixels 4q .. 4q + 3) q = its index, + step, .., two of them in
// flight; a quad is one 16-byte load from a frame that begins on a 16-byte boundary and four 4-byte loads from one that does
// not (each array on its own: x and d need not agree), and the last n_pix % 4 pixels go one by one.  Quads count from the
// frame's first pixel, not from an address: which lane adds which difference, and in which order, depends on n_pix alone, so
// the sums in double come out the same bits for a frame wherever it lies - in the caller's tensor, in a staging buffer, in a
// gathered list of offenders.  No atomics: the lanes of a wave reduce by a butterfly of shuffles (a + b on both sides of an
// exchange: every lane ends with the same bits), the four waves through LDS in wave order, and the workgroup writes one
// record; k_frame_errors_fold adds a frame's records in piece order.
//   key   bits(|x - d|, float) << 32 | ~pixel: the maximum is the largest error at its first pixel
//   kmin, kmax   order keys of x (float_order_key: -0 is +0);  bad   x holds a NaN or an Inf
namespace {
struct ErrRecord { unsigned long long key, n_over; double sum, sum_sq; unsigned kmin, kmax, bad, pad; };
static_assert(sizeof(ErrRecord) == 48, "one record is 48 bytes");
__device__ inline void err_fold(ErrRecord &a, const ErrRecord &b)
{
    a.key = max(a.key, b.key); a.n_over += b.n_over; a.sum += b.sum; a.sum_sq += b.sum_sq;
    a.kmin = min(a.kmin, b.kmin); a.kmax = max(a.kmax, b.kmax); a.bad |= b.bad;
}
__global__ __launch_bounds__(256) void k_frame_errors(const float *__restrict__ x, const float *__restrict__ d, size_t n_pix,
                                                      const float *__restrict__ bound, ErrRecord *__restrict__ part)
{
    const float *__restrict__ xf = x + (size_t) blockIdx.y * n_pix, *__restrict__ df = d + (size_t) blockIdx.y * n_pix;
    const float lim = bound ? bound[blockIdx.y] : 0.0f;
    ErrRecord r{0, 0, 0.0, 0.0, ~0u, 0u, 0u, 0u};
    auto take = [&](float a, float b, size_t pixel) {
        if (isnan(a) || isinf(a)) r.bad = 1;
        const unsigned k = float_order_key(a);
        r.kmin = min(r.kmin, k);
        r.kmax = max(r.kmax, k);
        const float ab = fabsf(a - b);
        r.key = max(r.key, ((unsigned long long) __float_as_uint(ab) << 32) | (unsigned) ~(unsigned) pixel);
        if (bound && ab > lim) r.n_over++;
        const double e = (double) a - (double) b;
        r.sum += e;
        r.sum_sq += e * e;
    };
    auto take4 = [&](const f32x4 &a, const f32x4 &b, size_t q) {
        take(a.x, b.x, 4 * q); take(a.y, b.y, 4 * q + 1); take(a.z, b.z, 4 * q + 2); take(a.w, b.w, 4 * q + 3);
    };
    // (uniform over the workgroup: a frame's base address)
    const bool xv = ((uintptr_t) xf & 15) == 0, dv = ((uintptr_t) df & 15) == 0;
    auto quad = [](const float *p, bool vec, size_t q) {
        if (vec) return reinterpret_cast<const f32x4 *>(p)[q];
        const float *s = p + 4 * q;
        return f32x4{s[0], s[1], s[2], s[3]};
    };
    const size_t gid = (size_t) blockIdx.x * blockDim.x + threadIdx.x, step = (size_t) gridDim.x * blockDim.x, n4 = n_pix >> 2;
    size_t i = gid;
    for (; i + step < n4; i += 2 * step) {
        const f32x4 a0 = quad(xf, xv, i), a1 = quad(xf, xv, i + step), b0 = quad(df, dv, i), b1 = quad(df, dv, i + step);
        take4(a0, b0, i);
        take4(a1, b1, i + step);
    }
    if (i < n4) take4(quad(xf, xv, i), quad(df, dv, i), i);
    if (4 * n4 + gid < n_pix) take(xf[4 * n4 + gid], df[4 * n4 + gid], 4 * n4 + gid);
    for (int o = 32; o >= 1; o >>= 1) {
        ErrRecord t;
        t.key = __shfl_xor(r.key, o); t.n_over = __shfl_xor(r.n_over, o); t.sum = __shfl_xor(r.sum, o); t.sum_sq = __shfl_xor(r.sum_sq, o);
        t.kmin = (unsigned) __shfl_xor((int) r.kmin, o); t.kmax = (unsigned) __shfl_xor((int) r.kmax, o); t.bad = (unsigned) __shfl_xor((int) r.bad, o);
        err_fold(r, t);
    }
    __shared__ ErrRecord waves[4];
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) err_fold(r, waves[w]);
        part[(size_t) blockIdx.y * gridDim.x + blockIdx.x] = r;
    }
}
// out[f] = the records part[f][0 .. pieces) of frame f added in piece order; a lane per frame
__global__ __launch_bounds__(64) void k_frame_errors_fold(const ErrRecord *__restrict__ part, unsigned pieces, unsigned n, ErrRecord *__restrict__ out)
{
    const unsigned f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    ErrRecord r = part[(size_t) f * pieces];
    for (unsigned p = 1; p < pieces; p++) err_fold(r, part[(size_t) f * pieces + p]);
    out[f] = r;
}
// workgroups a frame of n_pix pixels is cut into: two quads in flight a lane make 2048 pixels a step
unsigned frame_error_pieces(size_t n_pix) { return (unsigned) std::min<size_t>(std::max<size_t>(1, n_pix / 4096), 64); }
}  // namespace
// report[f] for the n frames d_d against d_x (device, [n][n_pix], any 4-byte alignment), counting |x - d| > bound[f] (host, may
// be null) -> 0, or 2 when a frame of d_x holds a NaN or an Inf.  Two launches, the bounds up and the records down per 4096
// frames, on ctx's stream, which is waited for.  Device current, the context the caller's alone.
int frame_errors(ebcc_hip_ctx *ctx, const float *d_x, const float *d_d, size_t n, size_t n_pix, const float *bound, ebcc_hip_frame_error *report)
{
    constexpr size_t kFrames = 4096;
    const unsigned pieces = frame_error_pieces(n_pix);
    const size_t most = std::min(n, kFrames), need = most * ((pieces + 1) * sizeof(ErrRecord) + sizeof(float));
    ctx->errs.reserve(need, true, false);
    ErrRecord *d_part = (ErrRecord *) ctx->errs.d, *d_res = d_part + most * pieces, *h_res = (ErrRecord *) ctx->errs.h;
    float *d_bound = (float *) (d_res + most), *h_bound = (float *) (h_res + most);
    int rc = 0;
    for (size_t lo = 0; lo < n; lo += kFrames) {
        const size_t m = std::min(kFrames, n - lo);
        if (bound) {
            memcpy(h_bound, bound + lo, m * sizeof(float));
            EBCC_HIP_CHECK(hipMemcpyAsync(d_bound, h_bound, m * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        }
        {
            ScopedTiming timing("frame_errors", ctx->stream);
            hipLaunchKernelGGL(k_frame_errors, dim3(pieces, (unsigned) m), dim3(256), 0, ctx->stream, d_x + lo * n_pix, d_d + lo * n_pix, n_pix,
                               bound ? (const float *) d_bound : nullptr, d_part);
            hipLaunchKernelGGL(k_frame_errors_fold, dim3((unsigned) ((m + 63) / 64)), dim3(64), 0, ctx->stream, (const ErrRecord *) d_part, pieces, (unsigned) m, d_res);
        }
        EBCC_HIP_LAUNCH_CHECK();
        EBCC_HIP_CHECK(hipMemcpyAsync(h_res, d_res, m * sizeof(ErrRecord), hipMemcpyDeviceToHost, ctx->stream));
        wait_stream(ctx->stream);
        for (size_t f = 0; f < m; f++) {
            const ErrRecord &r = h_res[f];
            if (r.bad) rc = 2;
            report[lo + f] = ebcc_hip_frame_error{u2f((uint32_t) (r.key >> 32)), ~(uint32_t) r.key, r.n_over, r.sum, r.sum_sq,
                                                  float_of_order_key(r.kmin), float_of_order_key(r.kmax)};
        }
    }
    return rc;
}

// Statistics over time (include/ebcc_hip.h: ebcc_hip_time_stats): the items [.][n_pix] that `list` names - (item, bin) pairs -
// folded into the accumulators [n_bins][n_pix] of their bins.  A lane owns pixels and walks the list from its first entry to its
// last, one item after the other: acc = acc + x, nothing else ever adds to a sample's accumulators, so for every bin and pixel
// the order of the additions is the order of the list - frames never meet in a reduction tree, and there are no atomics.  The
// walk is time_walk.hpp's: the lane keeps the current bin's accumulators in registers, writes them back and loads the other
// bin's only when the bin changes; time_fold hands over the list grouped by bin (a stable sort: within a bin still in
// increasing item index, which is all the order rule fixes), so a batch costs one load and one store of every bin it names.
// A quad is one 16-byte load from an item that begins on a 16-byte boundary, four 4-byte loads from one that does not, four
// items in flight; the accumulators of a bin the same way, each array on its own.  Which lane adds a sample does not matter
// here: the additions of a pixel are one lane's, in list order, wherever the arrays lie.  An accumulator that is NULL is neither
// loaded nor stored; min and max then start at 0, and -0 leaves as +0 in every store.
namespace {
struct FoldAcc { double *sum, *sum_sq; float *mn, *mx; unsigned *over; float threshold; };
struct FoldEntry { unsigned item, bin; };
struct TimeFold {
    typedef FoldEntry Entry;
    template <int W> struct Lane {
        typedef FoldEntry Entry;
        struct Items { float x[W]; };
        const size_t n_pix, p0;
        const float *__restrict__ items;
        const FoldAcc &a;
        double s[W], s2[W];
        float lo[W], hi[W];
        unsigned ov[W], cur = walk::kNone;
        __device__ __forceinline__ Lane(size_t n_pix_, size_t p0_, const float *items_, const FoldAcc &a_) : n_pix(n_pix_), p0(p0_), items(items_), a(a_)
        {
#pragma unroll
            for (int i = 0; i < W; i++) { s[i] = 0.0; s2[i] = 0.0; lo[i] = 0.0f; hi[i] = 0.0f; ov[i] = 0u; }
        }
        __device__ __forceinline__ void load(const Entry &e, Items &it) const { walk::get<float, W>(items + (size_t) e.item * n_pix + p0, it.x); }
        __device__ __forceinline__ bool changed(const Entry &e) const { return e.bin != cur; }
        __device__ __forceinline__ bool held() const { return cur != walk::kNone; }
        __device__ __forceinline__ void get(const Entry &e)
        {
            const size_t at = (size_t) e.bin * n_pix + p0;
            if (a.sum) walk::get<double, W>(a.sum + at, s);
            if (a.sum_sq) walk::get<double, W>(a.sum_sq + at, s2);
            if (a.mn) walk::get<float, W>(a.mn + at, lo);
            if (a.mx) walk::get<float, W>(a.mx + at, hi);
            if (a.over) walk::get<unsigned, W>(a.over + at, ov);
            cur = e.bin;
        }
        __device__ __forceinline__ void put()
        {
            const size_t at = (size_t) cur * n_pix + p0;
#pragma unroll
            for (int i = 0; i < W; i++) { lo[i] = lo[i] + 0.0f; hi[i] = hi[i] + 0.0f; }      // (-0 -> +0)
            if (a.sum) walk::put<double, W>(a.sum + at, s);
            if (a.sum_sq) walk::put<double, W>(a.sum_sq + at, s2);
            if (a.mn) walk::put<float, W>(a.mn + at, lo);
            if (a.mx) walk::put<float, W>(a.mx + at, hi);
            if (a.over) walk::put<unsigned, W>(a.over + at, ov);
        }
        __device__ __forceinline__ void step(const Entry &, const Items &it)
        {
#pragma unroll
            for (int i = 0; i < W; i++) {
                const float v = it.x[i];
                const double d = (double) v;
                s[i] = s[i] + d;
                s2[i] = s2[i] + d * d;
                lo[i] = fminf(lo[i], v);
                hi[i] = fmaxf(hi[i], v);
                ov[i] += v > a.threshold ? 1u : 0u;
            }
        }
    };
};
__global__ __launch_bounds__(256) void k_time_fold(const float *__restrict__ items, size_t n_pix, const FoldEntry *__restrict__ list, unsigned m, FoldAcc a)
{
    walk::lanes<TimeFold>(n_pix, list, m, items, a);
}
}  // namespace
// The items of d_items [n][n_pix] (device, any 4-byte alignment) that `bin` names (host, null: all bin 0; EBCC_HIP_NO_BIN: the
// item is not read) folded into st's accumulators, in index order within every bin (binned_list, walk_list: time_walk.hpp).
// st.count is the caller's.  Device current, the context the caller's alone, st checked (time_stats_named).
void time_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n, size_t n_pix, const uint32_t *bin, const ebcc_hip_time_stats &st)
{
    const auto list = binned_list<FoldEntry>(n, bin, [](size_t k, uint32_t b) { return FoldEntry{(unsigned) k, b}; });
    if (list.empty()) return;
    const FoldAcc a{st.d_sum, st.d_sum_sq, st.d_min, st.d_max, st.d_over, st.threshold};
    walk_list(ctx, "time_fold", list, [&](const FoldEntry *d_list, unsigned m, size_t) {
        hipLaunchKernelGGL(k_time_fold, walk::grid(n_pix), dim3(256), 0, ctx->stream, d_items, n_pix, d_list, m, a);
    });
}

// Area statistics per item (include/ebcc_hip.h: ebcc_hip_area_stat, and the order rule stated there): the weighted sums, the
// minimum and the maximum of every region of every item, by the fold the header fixes - fold64 over a row's terms with groups
// of four columns, then fold64 over a region's rows one by one.  Two launches, a wave (not a workgroup: nothing is shared, no
// LDS, no barrier) per row of a region, then a wave per region:
//   k_area_rows   lane l takes the quads l, l + 64, .. of its row, two of them in flight, term after term in column order
//                 (p = p + t: the partial sum l of the rule), the last cols % 4 columns in the quad they fall in; then the
//                 butterfly of shuffles (a + b on both sides of an exchange: every lane ends with the same bits) and lane 0
//                 writes the row's record.  Quads count from the region's first column, not from an address: a full quad is
//                 one 16-byte load where the row of the region happens to begin on a 16-byte boundary and four 4-byte loads
//                 where it does not (samples and weights each on their own), which changes no term and no order.
//   k_area_fold   lane l adds the row records l, l + 64, .. of its region in row order, the same butterfly, one record out.
// The items are windows [win rows][pitch] of their frames with the origin (row0, col0); regions and weights are in frame
// coordinates.  Region, row and weight of a wave are wave-uniform (the wave's index goes through readfirstlane: the tables are
// read by scalar loads).  No atomics.  A pixel whose weight is 0 adds nothing - the same bytes as a term of +0.0, since a
// partial sum that starts at +0.0 never becomes -0.0.
namespace {
struct AreaRegion { unsigned row0, col0, rows, cols, first, pad; };    // first: the region's first row record within an item
struct AreaRec { double sum, sum_sq, over; float mn, mx; };
static_assert(sizeof(AreaRec) == 32 && sizeof(ebcc_hip_area_stat) == 32, "one record is 32 bytes");
struct AreaWeights { const double *row; const float *pix; unsigned width; int use_threshold; float threshold; };   // (device pointers)
__device__ inline void area_add(AreaRec &a, const AreaRec &b)
{
    a.sum = a.sum + b.sum; a.sum_sq = a.sum_sq + b.sum_sq; a.over = a.over + b.over;
    a.mn = fminf(a.mn, b.mn); a.mx = fmaxf(a.mx, b.mx);
}
// every lane of the wave ends with the fold of all 64 records; -0 leaves as +0
__device__ inline void area_butterfly(AreaRec &r)
{
    for (int o = 32; o >= 1; o >>= 1) {
        AreaRec t;
        t.sum = __shfl_xor(r.sum, o); t.sum_sq = __shfl_xor(r.sum_sq, o); t.over = __shfl_xor(r.over, o);
        t.mn = __shfl_xor(r.mn, o); t.mx = __shfl_xor(r.mx, o);
        area_add(r, t);
    }
    r.mn = r.mn + 0.0f; r.mx = r.mx + 0.0f;
}
// the largest r with regions[r].first <= job (regions[0].first == 0)
__device__ inline unsigned area_region_of(const AreaRegion *__restrict__ regions, unsigned n_regions, unsigned job)
{
    unsigned lo = 0, hi = n_regions;
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (regions[mid].first <= job) lo = mid; else hi = mid;
    }
    return lo;
}
// wave w of the grid: row record w % jobs of item w / jobs, for w < n_items * jobs
__global__ __launch_bounds__(256) void k_area_rows(AreaItems items, unsigned n_items, const AreaRegion *__restrict__ regions, unsigned n_regions,
                                                   unsigned jobs, AreaWeights wt, AreaRec *__restrict__ rows)
{
    const unsigned wave = (unsigned) __builtin_amdgcn_readfirstlane((int) (blockIdx.x * 4u + (threadIdx.x >> 6))), lane = threadIdx.x & 63u;
    if (wave >= n_items * jobs) return;
    const unsigned item = wave / jobs, job = wave - item * jobs;
    const AreaRegion reg = regions[area_region_of(regions, n_regions, job)];
    const unsigned row = reg.row0 + (job - reg.first);                                  // (of the frame)
    const float *__restrict__ xs = items.d + (size_t) item * items.stride + (size_t) (row - items.row0) * items.pitch + (reg.col0 - items.col0);
    const float *__restrict__ ws = wt.pix ? wt.pix + (size_t) row * wt.width + reg.col0 : nullptr;
    const double wr = wt.row ? wt.row[row] : 1.0;
    AreaRec r{0.0, 0.0, 0.0, __builtin_inff(), -__builtin_inff()};
    auto take = [&](float x, float wp) {
        const double w = wr * (double) wp;
        if (w != 0.0) {
            const double xd = (double) x;
            r.sum = r.sum + xd * w;
            r.sum_sq = r.sum_sq + (xd * xd) * w;
            r.over = r.over + (wt.use_threshold && x > wt.threshold ? w : 0.0);
            r.mn = fminf(r.mn, x);
            r.mx = fmaxf(r.mx, x);
        }
    };
    auto take4 = [&](const f32x4 &x, const f32x4 &w) { take(x.x, w.x); take(x.y, w.y); take(x.z, w.z); take(x.w, w.w); };
    // (uniform over the wave: where the row of the region begins)
    const bool xv = ((uintptr_t) xs & 15) == 0, wv = ((uintptr_t) ws & 15) == 0;
    auto quad = [](const float *p, bool vec, unsigned q) {
        if (!p) return f32x4{1.0f, 1.0f, 1.0f, 1.0f};
        if (vec) return reinterpret_cast<const f32x4 *>(p)[q];
        const float *s = p + 4 * (size_t) q;
        return f32x4{s[0], s[1], s[2], s[3]};
    };
    const unsigned n4 = reg.cols >> 2, tail = reg.cols & 3u;
    unsigned q = lane;
    for (; q + 64 < n4; q += 128) {
        const f32x4 x0 = quad(xs, xv, q), x1 = quad(xs, xv, q + 64), w0 = quad(ws, wv, q), w1 = quad(ws, wv, q + 64);
        take4(x0, w0);
        take4(x1, w1);
    }
    if (q < n4) take4(quad(xs, xv, q), quad(ws, wv, q));
    if (tail && lane == (n4 & 63u))                                                     // (quad n4 is this lane's last)
        for (unsigned c = 4 * n4; c < reg.cols; c++) take(xs[c], ws ? ws[c] : 1.0f);
    area_butterfly(r);
    if (lane == 0) rows[(size_t) item * jobs + job] = r;
}
// wave w of the grid: region w % n_regions of item w / n_regions, from its row records
__global__ __launch_bounds__(256) void k_area_fold(const AreaRec *__restrict__ rows, unsigned n_items, const AreaRegion *__restrict__ regions, unsigned n_regions,
                                                   unsigned jobs, AreaRec *__restrict__ out)
{
    const unsigned wave = (unsigned) __builtin_amdgcn_readfirstlane((int) (blockIdx.x * 4u + (threadIdx.x >> 6))), lane = threadIdx.x & 63u;
    if (wave >= n_items * n_regions) return;
    const unsigned item = wave / n_regions, g = wave - item * n_regions;
    const AreaRegion reg = regions[g];
    const AreaRec *__restrict__ mine = rows + (size_t) item * jobs + reg.first;
    AreaRec r{0.0, 0.0, 0.0, __builtin_inff(), -__builtin_inff()};
    for (unsigned j = lane; j < reg.rows; j += 64) area_add(r, mine[j]);
    area_butterfly(r);
    if (lane == 0) out[wave] = r;
}
// 1 into *bad when a weight of the box [row0, +rows) x [col0, +cols) of pix [.][width] is negative, a NaN or an Inf (every
// lane that finds one stores the same word)
__global__ __launch_bounds__(256) void k_area_weights_bad(const float *__restrict__ pix, unsigned width, unsigned row0, unsigned col0, unsigned rows, unsigned cols,
                                                          unsigned *__restrict__ bad)
{
    const size_t n = (size_t) rows * cols;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        const float w = pix[(size_t) (row0 + i / cols) * width + col0 + i % cols];
        if (!(w >= 0.0f) || isinf(w)) *bad = 1u;
    }
}
}  // namespace
// What ebcc_hip_area_check checks -> n_regions and the bounding box of the regions, or -1 with the message set.
long area_checked(const char *who, size_t height, size_t width, const ebcc_hip_area_spec *spec, ebcc_hip_region *bounding)
{
    if (!spec || !spec->regions) { set_error("%s: no spec, or no region list", who); return -1; }
    if (spec->n_regions < 1) { set_error("%s: n_regions must not be zero", who); return -1; }
    if (height < 1 || width < 1 || height > 2047 || width > 2047) { set_error("%s: unsupported geometry %zu x %zu", who, height, width); return -1; }
    size_t bytes = 0;
    if (spec->n_regions > (size_t) LONG_MAX || __builtin_mul_overflow(spec->n_regions, sizeof(AreaRegion) + sizeof(AreaRec), &bytes)) {
        set_error("%s: the size of the region table overflows", who);
        return -1;
    }
    if ((uintptr_t) spec->d_w_pix & 3) { set_error("%s: d_w_pix must be 4-byte aligned", who); return -1; }
    size_t r0 = height, c0 = width, r1 = 0, c1 = 0;
    for (size_t g = 0; g < spec->n_regions; g++) {
        const ebcc_hip_region &R = spec->regions[g];
        if (R.rows < 1 || R.cols < 1 || R.row0 >= height || R.col0 >= width || R.rows > height - R.row0 || R.cols > width - R.col0) {
            set_error("%s: region %zu, [%zu, +%zu) x [%zu, +%zu), is empty or not inside the %zu x %zu frame", who, g, R.row0, R.rows, R.col0, R.cols, height, width);
            return -1;
        }
        r0 = std::min(r0, R.row0); c0 = std::min(c0, R.col0); r1 = std::max(r1, R.row0 + R.rows); c1 = std::max(c1, R.col0 + R.cols);
    }
    if (spec->w_row)
        for (size_t r = 0; r < height; r++)
            if (!(spec->w_row[r] >= 0.0) || std::isinf(spec->w_row[r])) { set_error("%s: w_row[%zu] is negative, a NaN or an Inf", who, r); return -1; }
    if (bounding) *bounding = ebcc_hip_region{r0, c0, r1 - r0, c1 - c0};
    return (long) spec->n_regions;
}
// The device pass over the weights of the box `bb` -> true when one of them is negative, a NaN or an Inf.  On ctx's stream,
// which is waited for; the word lies in the context's record buffer.  Device current, the context the caller's alone.
bool area_weights_bad(ebcc_hip_ctx *ctx, const float *d_w_pix, size_t width, const ebcc_hip_region &bb)
{
    ctx->errs.reserve(256, true, false);
    unsigned *d_bad = (unsigned *) ctx->errs.d, *h_bad = (unsigned *) ctx->errs.h;
    EBCC_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(unsigned), ctx->stream));
    const size_t n = bb.rows * bb.cols;
    hipLaunchKernelGGL(k_area_weights_bad, dim3((unsigned) std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, ctx->stream, d_w_pix, (unsigned) width,
                       (unsigned) bb.row0, (unsigned) bb.col0, (unsigned) bb.rows, (unsigned) bb.cols, d_bad);
    EBCC_HIP_LAUNCH_CHECK();
    EBCC_HIP_CHECK(hipMemcpyAsync(h_bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    wait_stream(ctx->stream);
    return *h_bad != 0;
}
// out[k][g] (host, [n][n_regions]) for the n items and the regions of a checked spec (area_checked).  w_row and the region
// table go up through the context's pinned table (boxes_reserve); row records and records lie in the context's record buffer
// (ctx->errs), and no launch makes more than kAreaRecords of either: the regions are cut into groups of at most that many
// rows, the items of a group into runs of at most that many row records (at least one item).  The records of a run come home
// in one copy.  On ctx's stream, which is waited for.  Device current, the context the caller's alone.
constexpr size_t kAreaRecords = (size_t) 1 << 18;
void area_fold(ebcc_hip_ctx *ctx, const AreaItems &items, size_t n, size_t height, size_t width, const ebcc_hip_area_spec &spec, ebcc_hip_area_stat *out)
{
    const size_t R = spec.n_regions, row_bytes = spec.w_row ? height * sizeof(double) : 0;
    boxes_reserve(ctx, 1, row_bytes + R * sizeof(AreaRegion));
    AreaRegion *h_reg = (AreaRegion *) ((char *) ctx->boxes.h + row_bytes);
    const AreaRegion *d_reg = (const AreaRegion *) ((const char *) ctx->boxes.d + row_bytes);
    if (spec.w_row) memcpy(ctx->boxes.h, spec.w_row, row_bytes);
    // regions [g0, g0 + G) with J rows in all, at most kAreaRecords (a region has at most 2047), taken `run` items a time
    struct Group { size_t g0, G, J, run; };
    std::vector<Group> groups;
    size_t need = 0;
    auto close = [&](size_t g0, size_t g1, size_t J) {
        const size_t run = std::min(n, std::max<size_t>(1, kAreaRecords / J));
        groups.push_back(Group{g0, g1 - g0, J, run});
        need = std::max(need, run * (J + (g1 - g0)) * sizeof(AreaRec));
    };
    size_t g0 = 0, jobs = 0;
    for (size_t g = 0; g < R; g++) {
        const ebcc_hip_region &S = spec.regions[g];
        if (jobs + S.rows > kAreaRecords) { close(g0, g, jobs); g0 = g; jobs = 0; }
        h_reg[g] = AreaRegion{(unsigned) S.row0, (unsigned) S.col0, (unsigned) S.rows, (unsigned) S.cols, (unsigned) jobs, 0u};
        jobs += S.rows;
    }
    close(g0, R, jobs);
    EBCC_HIP_CHECK(hipMemcpyAsync(ctx->boxes.d, ctx->boxes.h, row_bytes + R * sizeof(AreaRegion), hipMemcpyHostToDevice, ctx->stream));
    ctx->errs.reserve(need, true, false);
    const AreaWeights wt{spec.w_row ? (const double *) ctx->boxes.d : nullptr, spec.d_w_pix, (unsigned) width, spec.use_threshold, spec.threshold};
    for (const Group &gr : groups) {
        AreaRec *d_rows = (AreaRec *) ctx->errs.d, *d_out = d_rows + gr.run * gr.J;
        const AreaRec *h_out = (const AreaRec *) ctx->errs.h;
        for (size_t lo = 0; lo < n; lo += gr.run) {
            const size_t m = std::min(gr.run, n - lo);
            AreaItems part = items;
            part.d += lo * items.stride;
            {
                ScopedTiming timing("area_fold", ctx->stream);
                hipLaunchKernelGGL(k_area_rows, dim3((unsigned) ((m * gr.J + 3) / 4)), dim3(256), 0, ctx->stream, part, (unsigned) m, d_reg + gr.g0, (unsigned) gr.G,
                                   (unsigned) gr.J, wt, d_rows);
                hipLaunchKernelGGL(k_area_fold, dim3((unsigned) ((m * gr.G + 3) / 4)), dim3(256), 0, ctx->stream, (const AreaRec *) d_rows, (unsigned) m, d_reg + gr.g0,
                                   (unsigned) gr.G, (unsigned) gr.J, d_out);
            }
            EBCC_HIP_LAUNCH_CHECK();
            EBCC_HIP_CHECK(hipMemcpyAsync(ctx->errs.h, d_out, m * gr.G * sizeof(AreaRec), hipMemcpyDeviceToHost, ctx->stream));
            wait_stream(ctx->stream);
            for (size_t k = 0; k < m; k++) memcpy(out + (lo + k) * R + gr.g0, h_out + k * gr.G, gr.G * sizeof(AreaRec));
        }
    }
}

// ---- the arguments of the statistics over time (include/ebcc_hip.h: ebcc_hip_time_stats; k_time_fold above)
// What ebcc_hip_time_stats_check checks: the accumulators alone (time_stats_shape: also what ebcc_hip_time_stats_init needs),
// then the window in a height x width frame and the bins -> the number of named frames, or -1 with the message set.
bool time_stats_shape(const char *who, const ebcc_hip_time_stats *st)
{
    if (!st || !st->count) { set_error("%s: no statistics, or no count array", who); return false; }
    if (st->n_bins < 1 || st->rows < 1 || st->cols < 1) { set_error("%s: n_bins, rows and cols must not be zero", who); return false; }
    if (!st->d_sum && !st->d_sum_sq && !st->d_min && !st->d_max && !st->d_over) { set_error("%s: every accumulator is NULL", who); return false; }
    if (((uintptr_t) st->d_sum & 7) || ((uintptr_t) st->d_sum_sq & 7)) { set_error("%s: d_sum and d_sum_sq must be 8-byte aligned", who); return false; }
    if (((uintptr_t) st->d_min & 3) || ((uintptr_t) st->d_max & 3) || ((uintptr_t) st->d_over & 3)) {
        set_error("%s: d_min, d_max and d_over must be 4-byte aligned", who);
        return false;
    }
    return accumulator_bytes_checked(who, st->rows, st->cols, st->n_bins, sizeof(double));
}
long time_stats_named(const char *who, size_t height, size_t width, const ebcc_hip_time_stats *st, const uint32_t *bin, size_t n_frames,
                      size_t row0, size_t col0)
{
    if (!time_stats_shape(who, st) || !frame_window_checked(who, height, width, row0, col0, st->rows, st->cols)) return -1;
    return bins_named(who, "frame", n_frames, bin, st->n_bins);
}

}  // namespace ebcc
