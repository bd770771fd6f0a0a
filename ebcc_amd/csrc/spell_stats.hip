// spell_stats.hip - the spell decode's own part: run lengths and event timing over time at every pixel - the check of the
// arguments, the kernel and its launcher (spell_stats.hpp).  Not in the timed encode or decode chain.  The rule is stated at
// ebcc_hip_spell_stats in include/ebcc_hip.h and restated at the kernel: that comment is the specification the tests check.
#include <climits>
#include "spell_stats.hpp"

namespace ebcc {

// The rule.  A step carries a sample x, a bin, a label `when` and a flag `fresh`.  For every bin and pixel the steps of the bin
// are taken in the order of the list, which is increasing step, one after the other:
//   e = below ? x < threshold : x > threshold                     (in float: a NaN is never an event and ends a run)
//   runs      if (fresh) run = 0;  run = e ? run + 1 : 0
//             if (run > longest) { longest = run; longest_end = when; }                        (strictly: the earliest of equal runs stays)
//             if (run == min_len) { spells += 1; spell_steps += min_len; } else if (run > min_len) spell_steps += 1
//   events    if (e) { events += 1; if (first == NO_STEP) first = when; last = when; }
//   extremes  if (x > max) { max = x; when_max = when; }   if (x < min) { min = x; when_min = when; }   (strictly, in float)
// -0 compares equal to +0 and +0 is stored, as k_time_fold stores it, and a sample that is not above the maximum so far leaves
// it alone as fmaxf does: min and max are the bytes of the reduce decode, events with below == 0 the bytes of its `over`.
// Everything is an integer or a float comparison.  The state - `run` included - lives in the accumulators, so nothing else is
// carried from a launch, a batch or a call to the next.
//
// k_spell_fold is k_time_fold (array_stats.hip) with a label and a flag to an entry: a lane owns a quad of pixels (4q .. 4q + 3,
// counted from the item's first pixel; the last n_pix % 4 pixels go one to a lane) and walks the list from its first entry to
// its last, four items in flight - one 16-byte load from an item that begins on a 16-byte boundary, four 4-byte loads from one
// that does not.  The lane keeps the current bin's accumulators in registers, writes them back and loads the other bin's only
// when the bin changes; spell_fold hands over the list grouped by bin (a stable sort: within a bin still in increasing step), so
// a batch costs one load and one store of every bin it names.  The state of a pixel is one lane's, in list order, wherever the
// arrays lie.  Everything that decides a branch between lanes - the entry, which arrays are there - is the same in all lanes
// (what depends on a sample is a select), and no index depends on a sample.  No LDS, no atomics, plain vector stores.
// An instance for every set of the three families - runs, events, extremes -, so that a call holds and executes only what it
// asked for.  Within an instance an array that is NULL is neither loaded nor stored; what the check guarantees - d_run under
// every runs array, d_longest under d_longest_end, d_max / d_min under their labels - is that no stored array depends on one
// that was not loaded.
namespace {
struct SpellAcc {
    unsigned *run, *longest, *longest_end, *spells, *spell_steps, *events, *first, *last;
    float *mn, *mx;
    unsigned *when_min, *when_max;
    float threshold;
    int below;
    unsigned min_len;
};
struct SpellEntry { unsigned item, bin, when, fresh; };
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <class T> struct SpellVec16;                              // the 16-byte vector of T
template <> struct SpellVec16<float> { typedef f32x4 type; };
template <> struct SpellVec16<unsigned> { typedef u32x4 type; };
// W words at p: as one 16-byte access where W == 4 and p is on a 16-byte boundary (the same answer in every lane of a
// workgroup's quads: they lie whole quads apart), else one by one
template <class T, int W> __device__ inline void spell_get(const T *p, T (&r)[W])
{
    typedef typename SpellVec16<T>::type V;
    if constexpr (W == 4) {
        if (((uintptr_t) p & 15) == 0) {
            const V q = *reinterpret_cast<const V *>(p);
#pragma unroll
            for (int i = 0; i < 4; i++) r[i] = q[i];
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) r[i] = p[i];
}
template <class T, int W> __device__ inline void spell_put(T *p, const T (&r)[W])
{
    typedef typename SpellVec16<T>::type V;
    if constexpr (W == 4) {
        if (((uintptr_t) p & 15) == 0) {
            V q;
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] = r[i];
            *reinterpret_cast<V *>(p) = q;
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) p[i] = r[i];
}
// the state of W pixels: only what the instance folds takes registers
template <bool ON, int W> struct SpellRuns { unsigned run[W], longest[W], longest_end[W], spells[W], spell_steps[W]; };
template <int W> struct SpellRuns<false, W> {};
template <bool ON, int W> struct SpellEvents { unsigned events[W], first[W], last[W]; };
template <int W> struct SpellEvents<false, W> {};
template <bool ON, int W> struct SpellExtremes { float lo[W], hi[W]; unsigned when_lo[W], when_hi[W]; };
template <int W> struct SpellExtremes<false, W> {};

// the pixels p0 .. p0 + W - 1 through the list
template <bool RUNS, bool EVT, bool EXT, int W>
__device__ inline void spell_fold_pixels(const float *__restrict__ items, size_t n_pix, size_t p0, const SpellEntry *__restrict__ list, unsigned m,
                                         const SpellAcc &a)
{
    constexpr unsigned kNone = 0xFFFFFFFFu;                         // no bin yet; EBCC_HIP_NO_STEP
    constexpr int kDepth = 4;                                       // items in flight
    SpellRuns<RUNS, W> r;
    SpellEvents<EVT, W> v;
    SpellExtremes<EXT, W> x;
#pragma unroll
    for (int i = 0; i < W; i++) {
        if constexpr (RUNS) { r.run[i] = 0u; r.longest[i] = 0u; r.longest_end[i] = kNone; r.spells[i] = 0u; r.spell_steps[i] = 0u; }
        if constexpr (EVT) { v.events[i] = 0u; v.first[i] = kNone; v.last[i] = kNone; }
        if constexpr (EXT) { x.lo[i] = __builtin_inff(); x.hi[i] = -__builtin_inff(); x.when_lo[i] = kNone; x.when_hi[i] = kNone; }
    }
    unsigned cur = kNone;
    auto get = [&](unsigned b) {
        const size_t at = (size_t) b * n_pix + p0;
        if constexpr (RUNS) {
            if (a.run) spell_get<unsigned, W>(a.run + at, r.run);
            if (a.longest) spell_get<unsigned, W>(a.longest + at, r.longest);
            if (a.longest_end) spell_get<unsigned, W>(a.longest_end + at, r.longest_end);
            if (a.spells) spell_get<unsigned, W>(a.spells + at, r.spells);
            if (a.spell_steps) spell_get<unsigned, W>(a.spell_steps + at, r.spell_steps);
        }
        if constexpr (EVT) {
            if (a.events) spell_get<unsigned, W>(a.events + at, v.events);
            if (a.first) spell_get<unsigned, W>(a.first + at, v.first);
            if (a.last) spell_get<unsigned, W>(a.last + at, v.last);
        }
        if constexpr (EXT) {
            if (a.mn) spell_get<float, W>(a.mn + at, x.lo);
            if (a.mx) spell_get<float, W>(a.mx + at, x.hi);
            if (a.when_min) spell_get<unsigned, W>(a.when_min + at, x.when_lo);
            if (a.when_max) spell_get<unsigned, W>(a.when_max + at, x.when_hi);
        }
    };
    auto put = [&](unsigned b) {
        const size_t at = (size_t) b * n_pix + p0;
        if constexpr (RUNS) {
            if (a.run) spell_put<unsigned, W>(a.run + at, r.run);
            if (a.longest) spell_put<unsigned, W>(a.longest + at, r.longest);
            if (a.longest_end) spell_put<unsigned, W>(a.longest_end + at, r.longest_end);
            if (a.spells) spell_put<unsigned, W>(a.spells + at, r.spells);
            if (a.spell_steps) spell_put<unsigned, W>(a.spell_steps + at, r.spell_steps);
        }
        if constexpr (EVT) {
            if (a.events) spell_put<unsigned, W>(a.events + at, v.events);
            if (a.first) spell_put<unsigned, W>(a.first + at, v.first);
            if (a.last) spell_put<unsigned, W>(a.last + at, v.last);
        }
        if constexpr (EXT) {
#pragma unroll
            for (int i = 0; i < W; i++) { x.lo[i] = x.lo[i] + 0.0f; x.hi[i] = x.hi[i] + 0.0f; }      // (-0 -> +0)
            if (a.mn) spell_put<float, W>(a.mn + at, x.lo);
            if (a.mx) spell_put<float, W>(a.mx + at, x.hi);
            if (a.when_min) spell_put<unsigned, W>(a.when_min + at, x.when_lo);
            if (a.when_max) spell_put<unsigned, W>(a.when_max + at, x.when_hi);
        }
    };
    for (unsigned j0 = 0; j0 < m; j0 += kDepth) {
        float s[kDepth][W];
#pragma unroll
        for (int j = 0; j < kDepth; j++)
            if (j0 + j < m) spell_get<float, W>(items + (size_t) list[j0 + j].item * n_pix + p0, s[j]);
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            if (j0 + j >= m) break;
            const SpellEntry &en = list[j0 + j];
            const unsigned b = en.bin, when = en.when;
            if (b != cur) {
                if (cur != kNone) put(cur);
                get(b);
                cur = b;
            }
            if constexpr (RUNS) {
                if (en.fresh) {
#pragma unroll
                    for (int i = 0; i < W; i++) r.run[i] = 0u;
                }
            }
#pragma unroll
            for (int i = 0; i < W; i++) {
                const float t = s[j][i];
                const bool e = a.below ? t < a.threshold : t > a.threshold;
                if constexpr (RUNS) {
                    const unsigned run = e ? r.run[i] + 1u : 0u;
                    r.run[i] = run;
                    if (run > r.longest[i]) { r.longest[i] = run; r.longest_end[i] = when; }
                    if (run == a.min_len) { r.spells[i] += 1u; r.spell_steps[i] += a.min_len; }
                    else if (run > a.min_len) r.spell_steps[i] += 1u;
                }
                if constexpr (EVT) {
                    if (e) {
                        v.events[i] += 1u;
                        if (v.first[i] == kNone) v.first[i] = when;
                        v.last[i] = when;
                    }
                }
                if constexpr (EXT) {
                    if (t > x.hi[i]) { x.hi[i] = t; x.when_hi[i] = when; }
                    if (t < x.lo[i]) { x.lo[i] = t; x.when_lo[i] = when; }
                }
            }
        }
    }
    if (cur != kNone) put(cur);
}
// a lane per quad of an item, then a lane per pixel of the last n_pix % 4
template <bool RUNS, bool EVT, bool EXT>
__global__ __launch_bounds__(256) void k_spell_fold(const float *__restrict__ items, size_t n_pix, const SpellEntry *__restrict__ list, unsigned m, SpellAcc a)
{
    const size_t u = (size_t) blockIdx.x * blockDim.x + threadIdx.x, n4 = n_pix >> 2;
    if (u < n4) spell_fold_pixels<RUNS, EVT, EXT, 4>(items, n_pix, 4 * u, list, m, a);
    else if (u - n4 < (n_pix & 3)) spell_fold_pixels<RUNS, EVT, EXT, 1>(items, n_pix, 4 * n4 + (u - n4), list, m, a);
}
bool spell_runs(const ebcc_hip_spell_stats &st) { return st.d_run || st.d_longest || st.d_longest_end || st.d_spells || st.d_spell_steps; }
bool spell_events(const ebcc_hip_spell_stats &st) { return st.d_events || st.d_first || st.d_last; }
bool spell_extremes(const ebcc_hip_spell_stats &st) { return st.d_min || st.d_max || st.d_when_min || st.d_when_max; }
}  // namespace

void spell_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n, size_t n_pix, const uint32_t *bin, const uint32_t *when, const uint8_t *fresh,
                const ebcc_hip_spell_stats &st)
{
    constexpr size_t kList = 65536;
    std::vector<SpellEntry> list;
    list.reserve(n);
    for (size_t k = 0; k < n; k++)
        if (!bin || bin[k] != EBCC_HIP_NO_BIN)
            list.push_back(SpellEntry{(unsigned) k, bin ? bin[k] : 0u, when ? when[k] : (unsigned) k, fresh && fresh[k] ? 1u : 0u});
    if (list.empty()) return;
    std::stable_sort(list.begin(), list.end(), [](const SpellEntry &p, const SpellEntry &q) { return p.bin < q.bin; });
    boxes_reserve(ctx, list.size(), sizeof(SpellEntry));
    memcpy(ctx->boxes.h, list.data(), list.size() * sizeof(SpellEntry));
    EBCC_HIP_CHECK(hipMemcpyAsync(ctx->boxes.d, ctx->boxes.h, list.size() * sizeof(SpellEntry), hipMemcpyHostToDevice, ctx->stream));
    const SpellAcc a{st.d_run, st.d_longest, st.d_longest_end, st.d_spells, st.d_spell_steps, st.d_events, st.d_first, st.d_last, st.d_min, st.d_max,
                     st.d_when_min, st.d_when_max, st.threshold, st.below, st.min_len};
    typedef void (*Kernel)(const float *, size_t, const SpellEntry *, unsigned, SpellAcc);
    static const Kernel kernels[8] = {nullptr, k_spell_fold<true, false, false>, k_spell_fold<false, true, false>, k_spell_fold<true, true, false>,
                                      k_spell_fold<false, false, true>, k_spell_fold<true, false, true>, k_spell_fold<false, true, true>,
                                      k_spell_fold<true, true, true>};
    const Kernel kernel = kernels[(spell_runs(st) ? 1 : 0) | (spell_events(st) ? 2 : 0) | (spell_extremes(st) ? 4 : 0)];
    const size_t lanes = (n_pix >> 2) + (n_pix & 3);
    {
        ScopedTiming timing("spell_fold", ctx->stream);
        // a run of entries is cut with its launch: the next launch loads what this one stored
        for (size_t lo = 0; lo < list.size(); lo += kList)
            hipLaunchKernelGGL(kernel, dim3((unsigned) ((lanes + 255) / 256)), dim3(256), 0, ctx->stream, d_items, n_pix,
                               (const SpellEntry *) ctx->boxes.d + lo, (unsigned) std::min(kList, list.size() - lo), a);
    }
    EBCC_HIP_LAUNCH_CHECK();
    wait_stream(ctx->stream);
}

// ---- the arguments of the spell statistics (include/ebcc_hip.h: ebcc_hip_spell_stats)
bool spell_stats_shape(const char *who, const ebcc_hip_spell_stats *st)
{
    if (!st || !st->count) { set_error("%s: no statistics, or no count array", who); return false; }
    if (st->n_bins < 1 || st->rows < 1 || st->cols < 1) { set_error("%s: n_bins, rows and cols must not be zero", who); return false; }
    const bool runs = spell_runs(*st), events = spell_events(*st);
    if (!runs && !events && !spell_extremes(*st)) { set_error("%s: every accumulator is NULL", who); return false; }
    const void *const arrays[] = {st->d_run, st->d_longest, st->d_longest_end, st->d_spells, st->d_spell_steps, st->d_events, st->d_first, st->d_last,
                                  st->d_min, st->d_max, st->d_when_min, st->d_when_max};
    for (const void *p : arrays)
        if ((uintptr_t) p & 3) { set_error("%s: every accumulator must be 4-byte aligned", who); return false; }
    if (runs && !st->d_run) { set_error("%s: d_longest, d_longest_end, d_spells and d_spell_steps need d_run", who); return false; }
    if (st->d_longest_end && !st->d_longest) { set_error("%s: d_longest_end needs d_longest", who); return false; }
    if ((st->d_spells || st->d_spell_steps) && st->min_len == 0) { set_error("%s: d_spells and d_spell_steps need a min_len of 1 at least", who); return false; }
    if (st->d_when_max && !st->d_max) { set_error("%s: d_when_max needs d_max", who); return false; }
    if (st->d_when_min && !st->d_min) { set_error("%s: d_when_min needs d_min", who); return false; }
    if ((runs || events) && std::isnan(st->threshold)) { set_error("%s: the threshold is a NaN", who); return false; }
    size_t bytes = 0;
    if (__builtin_mul_overflow(st->rows, st->cols, &bytes) || __builtin_mul_overflow(bytes, st->n_bins, &bytes) ||
        __builtin_mul_overflow(bytes, sizeof(uint32_t), &bytes)) { set_error("%s: the size of the accumulators overflows", who); return false; }
    return true;
}
long spell_stats_named(const char *who, size_t height, size_t width, const ebcc_hip_spell_stats *st, const uint32_t *bin, const uint32_t *when,
                       size_t n_steps, size_t row0, size_t col0)
{
    if (!spell_stats_shape(who, st)) return -1;
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
        if (when ? when[t] == EBCC_HIP_NO_STEP : t >= (size_t) EBCC_HIP_NO_STEP) { set_error("%s: the label of step %zu is EBCC_HIP_NO_STEP", who, t); return -1; }
        named++;
    }
    if (!named) { set_error("%s: no step is named", who); return -1; }
    return (long) named;
}

}  // namespace ebcc
