// pair_stats.hip - the pair decode's own part: co-moments and vector magnitude of two variables over time at every pixel - the
// check of the arguments, the kernel and its launcher (pair_stats.hpp).  Not in the timed encode or decode chain.  The rule is
// stated at ebcc_hip_pair_stats in include/ebcc_hip.h and restated at the kernel: that comment is the specification the tests
// check.
#include <climits>
#include "pair_stats.hpp"
#include "time_walk.hpp"

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
// k_pair_fold is the walk of time_walk.hpp with two items to an entry: kDepth entries - twice as many items - in flight, one
// 16-byte load from an item that begins on a 16-byte boundary, four 4-byte loads from one that does not, decided for x and for y
// each on their own.  The lane keeps the current bin's accumulators in registers, writes them back and loads the other bin's
// only when the bin changes; pair_fold hands over the list grouped by bin (a stable sort: within a bin still in increasing
// step), so a batch costs one load and one store of every bin it names.  Which lane adds a sample does not matter: the
// additions of a pixel are one lane's, in list order, wherever the arrays lie.  Everything that decides a branch - the entry,
// which arrays are there - is the same in all lanes, and no index depends on a sample.  No LDS, no atomics, plain vector stores.
// Three instances, so that a call carries only what it asked for: MOM (the five co-moments: no square root is executed, no
// magnitude accumulator held), MAG (sum, maximum and count of the magnitude: no co-moment held) and both.  Within an instance
// an array that is NULL is neither loaded nor stored.
namespace {
struct PairAcc { double *sx, *sy, *sxx, *syy, *sxy, *smag; float *mx; unsigned *ov; float threshold; };
struct PairEntry { unsigned x, y, bin; };                           // items of the x and of the y base, and the step's bin
// the accumulators of W pixels: only what the instance folds takes registers
template <bool ON, int W> struct PairMoments { double sx[W], sy[W], sxx[W], syy[W], sxy[W]; };
template <int W> struct PairMoments<false, W> {};
template <bool ON, int W> struct PairMagnitude { double sm[W]; float mx[W]; unsigned ov[W]; };
template <int W> struct PairMagnitude<false, W> {};

template <bool MOM, bool MAG> struct PairFold {
    typedef PairEntry Entry;
    template <int W> struct Lane {
        typedef PairEntry Entry;
        struct Items { float x[W], y[W]; };
        const size_t n_pix, p0;
        const float *__restrict__ xs, *__restrict__ ys;
        const PairAcc &a;
        PairMoments<MOM, W> c;
        PairMagnitude<MAG, W> g;
        unsigned cur = walk::kNone;
        __device__ __forceinline__ Lane(size_t n_pix_, size_t p0_, const float *xs_, const float *ys_, const PairAcc &a_)
            : n_pix(n_pix_), p0(p0_), xs(xs_), ys(ys_), a(a_)
        {
#pragma unroll
            for (int i = 0; i < W; i++) {
                if constexpr (MOM) { c.sx[i] = 0.0; c.sy[i] = 0.0; c.sxx[i] = 0.0; c.syy[i] = 0.0; c.sxy[i] = 0.0; }
                if constexpr (MAG) { g.sm[i] = 0.0; g.mx[i] = 0.0f; g.ov[i] = 0u; }
            }
        }
        __device__ __forceinline__ void load(const Entry &e, Items &it) const
        {
            walk::get<float, W>(xs + (size_t) e.x * n_pix + p0, it.x);
            walk::get<float, W>(ys + (size_t) e.y * n_pix + p0, it.y);
        }
        __device__ __forceinline__ bool changed(const Entry &e) const { return e.bin != cur; }
        __device__ __forceinline__ bool held() const { return cur != walk::kNone; }
        __device__ __forceinline__ void get(const Entry &e)
        {
            const size_t at = (size_t) e.bin * n_pix + p0;
            if constexpr (MOM) {
                if (a.sx) walk::get<double, W>(a.sx + at, c.sx);
                if (a.sy) walk::get<double, W>(a.sy + at, c.sy);
                if (a.sxx) walk::get<double, W>(a.sxx + at, c.sxx);
                if (a.syy) walk::get<double, W>(a.syy + at, c.syy);
                if (a.sxy) walk::get<double, W>(a.sxy + at, c.sxy);
            }
            if constexpr (MAG) {
                if (a.smag) walk::get<double, W>(a.smag + at, g.sm);
                if (a.mx) walk::get<float, W>(a.mx + at, g.mx);
                if (a.ov) walk::get<unsigned, W>(a.ov + at, g.ov);
            }
            cur = e.bin;
        }
        __device__ __forceinline__ void put()
        {
            const size_t at = (size_t) cur * n_pix + p0;
            if constexpr (MOM) {
                if (a.sx) walk::put<double, W>(a.sx + at, c.sx);
                if (a.sy) walk::put<double, W>(a.sy + at, c.sy);
                if (a.sxx) walk::put<double, W>(a.sxx + at, c.sxx);
                if (a.syy) walk::put<double, W>(a.syy + at, c.syy);
                if (a.sxy) walk::put<double, W>(a.sxy + at, c.sxy);
            }
            if constexpr (MAG) {
                if (a.smag) walk::put<double, W>(a.smag + at, g.sm);
                if (a.mx) walk::put<float, W>(a.mx + at, g.mx);
                if (a.ov) walk::put<unsigned, W>(a.ov + at, g.ov);
            }
        }
        __device__ __forceinline__ void step(const Entry &, const Items &it)
        {
#pragma unroll
            for (int i = 0; i < W; i++) {
                const double u = (double) it.x[i], v = (double) it.y[i];
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
    };
};
template <bool MOM, bool MAG>
__global__ __launch_bounds__(256) void k_pair_fold(const float *__restrict__ xs, const float *__restrict__ ys, size_t n_pix,
                                                   const PairEntry *__restrict__ list, unsigned m, PairAcc a)
{
    walk::lanes<PairFold<MOM, MAG>>(n_pix, list, m, xs, ys, a);
}
}  // namespace

void pair_fold(ebcc_hip_ctx *ctx, const float *d_x, const float *d_y, bool interleaved, size_t n, size_t n_pix, const uint32_t *bin,
               const ebcc_hip_pair_stats &st)
{
    const auto list = binned_list<PairEntry>(n, bin, [&](size_t k, uint32_t b) {
        return interleaved ? PairEntry{(unsigned) (2 * k), (unsigned) (2 * k + 1), b} : PairEntry{(unsigned) k, (unsigned) k, b};
    });
    if (list.empty()) return;
    const PairAcc a{st.d_sum_x, st.d_sum_y, st.d_sum_xx, st.d_sum_yy, st.d_sum_xy, st.d_sum_mag, st.d_max_mag, st.d_over_mag, st.threshold};
    const bool mom = st.d_sum_x || st.d_sum_y || st.d_sum_xx || st.d_sum_yy || st.d_sum_xy, mag = st.d_sum_mag || st.d_max_mag || st.d_over_mag;
    const auto kernel = mom && mag ? k_pair_fold<true, true> : mom ? k_pair_fold<true, false> : k_pair_fold<false, true>;
    walk_list(ctx, "pair_fold", list, [&](const PairEntry *d_list, unsigned m, size_t) {
        hipLaunchKernelGGL(kernel, walk::grid(n_pix), dim3(256), 0, ctx->stream, d_x, d_y, n_pix, d_list, m, a);
    });
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
    return accumulator_bytes_checked(who, st->rows, st->cols, st->n_bins, sizeof(double));
}
long pair_stats_named(const char *who, size_t height, size_t width, const ebcc_hip_pair_stats *st, const uint32_t *bin, size_t n_steps, size_t row0,
                      size_t col0)
{
    if (!pair_stats_shape(who, st) || !frame_window_checked(who, height, width, row0, col0, st->rows, st->cols)) return -1;
    return bins_named(who, "step", n_steps, bin, st->n_bins);
}

}  // namespace ebcc
