// pair_stats.hip - the pair decode's own part: co-moments and vector magnitude of two variables over time at every pixel - the
// check of the arguments, the kernel and its launcher (pair_stats.hpp).  Not in the timed encode or decode chain.  The rule is
// stated at ebcc_hip_pair_stats in include/ebcc_hip.h and restated at the kernel: that comment is the specification the tests
// check.
#include <climits>
#include "pair_stats.hpp"

namespace ebcc {

// The rule.  Step t pairs x[t] with y[t].  For every bin and pixel the steps of the bin are taken in the order of the list,
// which is increasing step, one after the other, with a = (double) x and b = (double) y:
//   sum_x = sum_x + a;  sum_y = sum_y + b;  sum_xx = sum_xx + a * a;  sum_yy = sum_yy + b * b;  sum_xy = sum_xy + a * b
//   m = sqrtf((float) (a * a + b * b));  sum_mag = sum_mag + (double) m;  max_mag = fmaxf(max_mag, m);  over_mag += m > threshold
// A product of two widened floats is exact in double; a * a + b * b rounds once (to double: -ffp-contract=off, no FMA is formed -
// one would round the same sum once as well), the conversion to float rounds to nearest even, and the square root is the
// correctly rounded one (-fhip-fp32-correctly-rounded-divide-sqrt, which the whole library is built with).  Nothing else ever
// adds to an accumulator: no atomics, and steps never meet in a reduction tree.
//
// k_pair_fold is k_time_fold (array_stats.hip) with two items to an entry: a lane owns a quad of pixels (4q .. 4q + 3, counted
// from the item's first pixel; the last n_pix % 4 pixels go one to a lane) and walks the list from its first entry to its last,
// kDepth entries - twice as many items - in flight: one 16-byte load from an item that begins on a 16-byte boundary, four
// 4-byte loads from one that does not, decided for x and for y each on their own.  The lane keeps the current bin's
// accumulators in registers, writes them back and loads the other bin's only when the bin changes; pair_fold hands over the
// list grouped by bin (a stable sort: within a bin still in increasing step), so a batch costs one load and one store of every
// bin it names.  Which lane adds a sample does not matter: the additions of a pixel are one lane's, in list order, wherever the
// arrays lie.  Everything that decides a branch - the entry, which arrays are there - is the same in all lanes, and no index
// depends on a sample.  No LDS, no atomics, plain vector stores.
// Three instances, so that a call carries only what it asked for: MOM (the five co-moments: no square root is executed, no
// magnitude accumulator held), MAG (sum, maximum and count of the magnitude: no co-moment held) and both.  Within an instance
// an array that is NULL is neither loaded nor stored.
namespace {
struct PairAcc { double *sx, *sy, *sxx, *syy, *sxy, *smag; float *mx; unsigned *ov; float threshold; };
struct PairEntry { unsigned x, y, bin; };                           // items of the x and of the y base, and the step's bin
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <class T> struct PairVec16;                               // the 16-byte vector of T
template <> struct PairVec16<double> { typedef f64x2 type; };
template <> struct PairVec16<float> { typedef f32x4 type; };
template <> struct PairVec16<unsigned> { typedef u32x4 type; };
// W samples at p: as 16-byte accesses where W == 4 and p is on a 16-byte boundary (the same answer in every lane of a
// workgroup's quads: they lie whole quads apart), else one by one
template <class T, int W> __device__ inline void pair_get(const T *p, T (&r)[W])
{
    typedef typename PairVec16<T>::type V;
    constexpr int per = 16 / sizeof(T);
    if constexpr (W == 4) {
        if (((uintptr_t) p & 15) == 0) {
#pragma unroll
            for (int v = 0; v < W / per; v++) {
                const V q = reinterpret_cast<const V *>(p)[v];
#pragma unroll
                for (int i = 0; i < per; i++) r[v * per + i] = q[i];
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) r[i] = p[i];
}
template <class T, int W> __device__ inline void pair_put(T *p, const T (&r)[W])
{
    typedef typename PairVec16<T>::type V;
    constexpr int per = 16 / sizeof(T);
    if constexpr (W == 4) {
        if (((uintptr_t) p & 15) == 0) {
#pragma unroll
            for (int v = 0; v < W / per; v++) {
                V q;
#pragma unroll
                for (int i = 0; i < per; i++) q[i] = r[v * per + i];
                reinterpret_cast<V *>(p)[v] = q;
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) p[i] = r[i];
}
// the accumulators of W pixels: only what the instance folds takes registers
template <bool ON, int W> struct PairMoments { double sx[W], sy[W], sxx[W], syy[W], sxy[W]; };
template <int W> struct PairMoments<false, W> {};
template <bool ON, int W> struct PairMagnitude { double sm[W]; float mx[W]; unsigned ov[W]; };
template <int W> struct PairMagnitude<false, W> {};

// the pixels p0 .. p0 + W - 1 through the list
template <bool MOM, bool MAG, int W>
__device__ inline void pair_fold_pixels(const float *__restrict__ xs, const float *__restrict__ ys, size_t n_pix, size_t p0,
                                        const PairEntry *__restrict__ list, unsigned m, const PairAcc &a)
{
    constexpr unsigned kNone = 0xFFFFFFFFu;
    constexpr int kDepth = 4;                                       // entries in flight: an x and a y item each
    PairMoments<MOM, W> c;
    PairMagnitude<MAG, W> g;
#pragma unroll
    for (int i = 0; i < W; i++) {
        if constexpr (MOM) { c.sx[i] = 0.0; c.sy[i] = 0.0; c.sxx[i] = 0.0; c.syy[i] = 0.0; c.sxy[i] = 0.0; }
        if constexpr (MAG) { g.sm[i] = 0.0; g.mx[i] = 0.0f; g.ov[i] = 0u; }
    }
    unsigned cur = kNone;
    auto get = [&](unsigned b) {
        const size_t at = (size_t) b * n_pix + p0;
        if constexpr (MOM) {
            if (a.sx) pair_get<double, W>(a.sx + at, c.sx);
            if (a.sy) pair_get<double, W>(a.sy + at, c.sy);
            if (a.sxx) pair_get<double, W>(a.sxx + at, c.sxx);
            if (a.syy) pair_get<double, W>(a.syy + at, c.syy);
            if (a.sxy) pair_get<double, W>(a.sxy + at, c.sxy);
        }
        if constexpr (MAG) {
            if (a.smag) pair_get<double, W>(a.smag + at, g.sm);
            if (a.mx) pair_get<float, W>(a.mx + at, g.mx);
            if (a.ov) pair_get<unsigned, W>(a.ov + at, g.ov);
        }
    };
    auto put = [&](unsigned b) {
        const size_t at = (size_t) b * n_pix + p0;
        if constexpr (MOM) {
            if (a.sx) pair_put<double, W>(a.sx + at, c.sx);
            if (a.sy) pair_put<double, W>(a.sy + at, c.sy);
            if (a.sxx) pair_put<double, W>(a.sxx + at, c.sxx);
            if (a.syy) pair_put<double, W>(a.syy + at, c.syy);
            if (a.sxy) pair_put<double, W>(a.sxy + at, c.sxy);
        }
        if constexpr (MAG) {
            if (a.smag) pair_put<double, W>(a.smag + at, g.sm);
            if (a.mx) pair_put<float, W>(a.mx + at, g.mx);
            if (a.ov) pair_put<unsigned, W>(a.ov + at, g.ov);
        }
    };
    for (unsigned j0 = 0; j0 < m; j0 += kDepth) {
        float x[kDepth][W], y[kDepth][W];
#pragma unroll
        for (int j = 0; j < kDepth; j++)
            if (j0 + j < m) {
                pair_get<float, W>(xs + (size_t) list[j0 + j].x * n_pix + p0, x[j]);
                pair_get<float, W>(ys + (size_t) list[j0 + j].y * n_pix + p0, y[j]);
            }
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            if (j0 + j >= m) break;
            const unsigned b = list[j0 + j].bin;
            if (b != cur) {
                if (cur != kNone) put(cur);
                get(b);
                cur = b;
            }
#pragma unroll
            for (int i = 0; i < W; i++) {
                const double u = (double) x[j][i], v = (double) y[j][i];
                const double uu = u * u, vv = v * v;                // (exact)
                if constexpr (MOM) {
                    c.sx[i] = c.sx[i] + u;
                    c.sy[i] = c.sy[i] + v;
                    c.sxx[i] = c.sxx[i] + uu;
                    c.syy[i] = c.syy[i] + vv;
                    c.sxy[i] = c.sxy[i] + u * v;
                }
                if constexpr (MAG) {
                    const float mag = sqrtf((float) (uu + vv));     // one rounding to double, one to float, the correctly rounded root
                    g.sm[i] = g.sm[i] + (double) mag;
                    g.mx[i] = fmaxf(g.mx[i], mag);
                    g.ov[i] += mag > a.threshold ? 1u : 0u;
                }
            }
        }
    }
    if (cur != kNone) put(cur);
}
// a lane per quad of an item, then a lane per pixel of the last n_pix % 4
template <bool MOM, bool MAG>
__global__ __launch_bounds__(256) void k_pair_fold(const float *__restrict__ xs, const float *__restrict__ ys, size_t n_pix,
                                                   const PairEntry *__restrict__ list, unsigned m, PairAcc a)
{
    const size_t u = (size_t) blockIdx.x * blockDim.x + threadIdx.x, n4 = n_pix >> 2;
    if (u < n4) pair_fold_pixels<MOM, MAG, 4>(xs, ys, n_pix, 4 * u, list, m, a);
    else if (u - n4 < (n_pix & 3)) pair_fold_pixels<MOM, MAG, 1>(xs, ys, n_pix, 4 * n4 + (u - n4), list, m, a);
}
}  // namespace

void pair_fold(ebcc_hip_ctx *ctx, const float *d_x, const float *d_y, bool interleaved, size_t n, size_t n_pix, const uint32_t *bin,
               const ebcc_hip_pair_stats &st)
{
    constexpr size_t kList = 65536;
    std::vector<PairEntry> list;
    list.reserve(n);
    for (size_t k = 0; k < n; k++)
        if (!bin || bin[k] != EBCC_HIP_NO_BIN)
            list.push_back(interleaved ? PairEntry{(unsigned) (2 * k), (unsigned) (2 * k + 1), bin ? bin[k] : 0u} : PairEntry{(unsigned) k, (unsigned) k, bin ? bin[k] : 0u});
    if (list.empty()) return;
    std::stable_sort(list.begin(), list.end(), [](const PairEntry &p, const PairEntry &q) { return p.bin < q.bin; });
    boxes_reserve(ctx, list.size(), sizeof(PairEntry));
    memcpy(ctx->boxes.h, list.data(), list.size() * sizeof(PairEntry));
    EBCC_HIP_CHECK(hipMemcpyAsync(ctx->boxes.d, ctx->boxes.h, list.size() * sizeof(PairEntry), hipMemcpyHostToDevice, ctx->stream));
    const PairAcc a{st.d_sum_x, st.d_sum_y, st.d_sum_xx, st.d_sum_yy, st.d_sum_xy, st.d_sum_mag, st.d_max_mag, st.d_over_mag, st.threshold};
    const bool mom = st.d_sum_x || st.d_sum_y || st.d_sum_xx || st.d_sum_yy || st.d_sum_xy, mag = st.d_sum_mag || st.d_max_mag || st.d_over_mag;
    const auto kernel = mom && mag ? k_pair_fold<true, true> : mom ? k_pair_fold<true, false> : k_pair_fold<false, true>;
    const size_t lanes = (n_pix >> 2) + (n_pix & 3);
    {
        ScopedTiming timing("pair_fold", ctx->stream);
        // a run of entries is cut with its launch: the next launch loads what this one stored
        for (size_t lo = 0; lo < list.size(); lo += kList)
            hipLaunchKernelGGL(kernel, dim3((unsigned) ((lanes + 255) / 256)), dim3(256), 0, ctx->stream, d_x, d_y, n_pix,
                               (const PairEntry *) ctx->boxes.d + lo, (unsigned) std::min(kList, list.size() - lo), a);
    }
    EBCC_HIP_LAUNCH_CHECK();
    wait_stream(ctx->stream);
}

// ---- the arguments of the pair statistics (include/ebcc_hip.h: ebcc_hip_pair_stats)
bool pair_stats_shape(const char *who, const ebcc_hip_pair_stats *st)
{
    if (!st || !st->count) { set_error("%s: no statistics, or no count array", who); return false; }
    if (st->n_bins < 1 || st->rows < 1 || st->cols < 1) { set_error("%s: n_bins, rows and cols must not be zero", who); return false; }
    double *const doubles[] = {st->d_sum_x, st->d_sum_y, st->d_sum_xx, st->d_sum_yy, st->d_sum_xy, st->d_sum_mag};
    bool any = st->d_max_mag || st->d_over_mag;
    for (const double *p : doubles) {
        any = any || p;
        if ((uintptr_t) p & 7) { set_error("%s: d_sum_x, d_sum_y, d_sum_xx, d_sum_yy, d_sum_xy and d_sum_mag must be 8-byte aligned", who); return false; }
    }
    if (!any) { set_error("%s: every accumulator is NULL", who); return false; }
    if (((uintptr_t) st->d_max_mag & 3) || ((uintptr_t) st->d_over_mag & 3)) { set_error("%s: d_max_mag and d_over_mag must be 4-byte aligned", who); return false; }
    if (st->d_over_mag && std::isnan(st->threshold)) { set_error("%s: the threshold is a NaN", who); return false; }
    size_t bytes = 0;
    if (__builtin_mul_overflow(st->rows, st->cols, &bytes) || __builtin_mul_overflow(bytes, st->n_bins, &bytes) ||
        __builtin_mul_overflow(bytes, sizeof(double), &bytes)) { set_error("%s: the size of the accumulators overflows", who); return false; }
    return true;
}
long pair_stats_named(const char *who, size_t height, size_t width, const ebcc_hip_pair_stats *st, const uint32_t *bin, size_t n_steps, size_t row0,
                      size_t col0)
{
    if (!pair_stats_shape(who, st)) return -1;
    if (height < 1 || width < 1 || height > 2047 || width > 2047) { set_error("%s: unsupported geometry %zu x %zu", who, height, width); return -1; }
    if (row0 >= height || col0 >= width || st->rows > height - row0 || st->cols > width - col0) {
        set_error("%s: the window [%zu, +%zu) x [%zu, +%zu) is not inside the %zu x %zu frame", who, row0, st->rows, col0, st->cols, height, width);
        return -1;
    }
    if (n_steps > (size_t) LONG_MAX) { set_error("%s: too many steps", who); return -1; }
    size_t named = 0;
    for (size_t t = 0; t < n_steps; t++) {
        const uint32_t b = bin ? bin[t] : 0u;
        if (b == EBCC_HIP_NO_BIN) continue;
        if (b >= st->n_bins) { set_error("%s: step %zu names bin %u of %zu", who, t, b, st->n_bins); return -1; }
        named++;
    }
    if (!named) { set_error("%s: no step is named", who); return -1; }
    return (long) named;
}

}  // namespace ebcc
