// spell_stats.hip - the spell decode's own part: run lengths and event timing over time at every pixel - the check of the
// arguments, the kernel and its launcher (spell_stats.hpp).  Not in the timed encode or decode chain.  The rule is stated at
// ebcc_hip_spell_stats in include/ebcc_hip.h and restated at the kernel: that comment is the specification the tests check.
#include <climits>
#include "spell_stats.hpp"
#include "time_walk.hpp"

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
// k_spell_fold is the walk of time_walk.hpp with a label and a flag to an entry.  The lane keeps the current bin's accumulators
// in registers, writes them back and loads the other bin's only when the bin changes; spell_fold hands over the list grouped by
// bin (a stable sort: within a bin still in increasing step), so a batch costs one load and one store of every bin it names.
// The state of a pixel is one lane's, in list order, wherever the arrays lie.  Everything that decides a branch between lanes -
// the entry, which arrays are there - is the same in all lanes (what depends on a sample is a select), and no index depends on
// a sample.  No LDS, no atomics, plain vector stores.
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
// the state of W pixels: only what the instance folds takes registers
template <bool ON, int W> struct SpellRuns { unsigned run[W], longest[W], longest_end[W], spells[W], spell_steps[W]; };
template <int W> struct SpellRuns<false, W> {};
template <bool ON, int W> struct SpellEvents { unsigned events[W], first[W], last[W]; };
template <int W> struct SpellEvents<false, W> {};
template <bool ON, int W> struct SpellExtremes { float lo[W], hi[W]; unsigned when_lo[W], when_hi[W]; };
template <int W> struct SpellExtremes<false, W> {};

template <bool RUNS, bool EVT, bool EXT> struct SpellFold {
    typedef SpellEntry Entry;
    template <int W> struct Lane {
        typedef SpellEntry Entry;
        struct Items { float s[W]; };
        static constexpr unsigned kNoStep = 0xFFFFFFFFu;            // EBCC_HIP_NO_STEP
        const size_t n_pix, p0;
        const float *__restrict__ items;
        const SpellAcc &a;
        SpellRuns<RUNS, W> r;
        SpellEvents<EVT, W> v;
        SpellExtremes<EXT, W> x;
        unsigned cur = walk::kNone;
        __device__ __forceinline__ Lane(size_t n_pix_, size_t p0_, const float *items_, const SpellAcc &a_) : n_pix(n_pix_), p0(p0_), items(items_), a(a_)
        {
#pragma unroll
            for (int i = 0; i < W; i++) {
                if constexpr (RUNS) { r.run[i] = 0u; r.longest[i] = 0u; r.longest_end[i] = kNoStep; r.spells[i] = 0u; r.spell_steps[i] = 0u; }
                if constexpr (EVT) { v.events[i] = 0u; v.first[i] = kNoStep; v.last[i] = kNoStep; }
                if constexpr (EXT) { x.lo[i] = __builtin_inff(); x.hi[i] = -__builtin_inff(); x.when_lo[i] = kNoStep; x.when_hi[i] = kNoStep; }
            }
        }
        __device__ __forceinline__ void load(const Entry &e, Items &it) const { walk::get<float, W>(items + (size_t) e.item * n_pix + p0, it.s); }
        __device__ __forceinline__ bool changed(const Entry &e) const { return e.bin != cur; }
        __device__ __forceinline__ bool held() const { return cur != walk::kNone; }
        __device__ __forceinline__ void get(const Entry &e)
        {
            const size_t at = (size_t) e.bin * n_pix + p0;
            if constexpr (RUNS) {
                if (a.run) walk::get<unsigned, W>(a.run + at, r.run);
                if (a.longest) walk::get<unsigned, W>(a.longest + at, r.longest);
                if (a.longest_end) walk::get<unsigned, W>(a.longest_end + at, r.longest_end);
                if (a.spells) walk::get<unsigned, W>(a.spells + at, r.spells);
                if (a.spell_steps) walk::get<unsigned, W>(a.spell_steps + at, r.spell_steps);
            }
            if constexpr (EVT) {
                if (a.events) walk::get<unsigned, W>(a.events + at, v.events);
                if (a.first) walk::get<unsigned, W>(a.first + at, v.first);
                if (a.last) walk::get<unsigned, W>(a.last + at, v.last);
            }
            if constexpr (EXT) {
                if (a.mn) walk::get<float, W>(a.mn + at, x.lo);
                if (a.mx) walk::get<float, W>(a.mx + at, x.hi);
                if (a.when_min) walk::get<unsigned, W>(a.when_min + at, x.when_lo);
                if (a.when_max) walk::get<unsigned, W>(a.when_max + at, x.when_hi);
            }
            cur = e.bin;
        }
        __device__ __forceinline__ void put()
        {
            const size_t at = (size_t) cur * n_pix + p0;
            if constexpr (RUNS) {
                if (a.run) walk::put<unsigned, W>(a.run + at, r.run);
                if (a.longest) walk::put<unsigned, W>(a.longest + at, r.longest);
                if (a.longest_end) walk::put<unsigned, W>(a.longest_end + at, r.longest_end);
                if (a.spells) walk::put<unsigned, W>(a.spells + at, r.spells);
                if (a.spell_steps) walk::put<unsigned, W>(a.spell_steps + at, r.spell_steps);
            }
            if constexpr (EVT) {
                if (a.events) walk::put<unsigned, W>(a.events + at, v.events);
                if (a.first) walk::put<unsigned, W>(a.first + at, v.first);
                if (a.last) walk::put<unsigned, W>(a.last + at, v.last);
            }
            if constexpr (EXT) {
#pragma unroll
                for (int i = 0; i < W; i++) { x.lo[i] = x.lo[i] + 0.0f; x.hi[i] = x.hi[i] + 0.0f; }      // (-0 -> +0)
                if (a.mn) walk::put<float, W>(a.mn + at, x.lo);
                if (a.mx) walk::put<float, W>(a.mx + at, x.hi);
                if (a.when_min) walk::put<unsigned, W>(a.when_min + at, x.when_lo);
                if (a.when_max) walk::put<unsigned, W>(a.when_max + at, x.when_hi);
            }
        }
        // (fresh: after the bin's state is loaded, before the sample)
        __device__ __forceinline__ void step(const Entry &en, const Items &it)
        {
            const unsigned when = en.when;
            // (local copies: on the members the conditional updates compile to branches, on locals to the selects of the rule)
            SpellRuns<RUNS, W> r = this->r;
            SpellEvents<EVT, W> v = this->v;
            SpellExtremes<EXT, W> x = this->x;
            if constexpr (RUNS) {
                if (en.fresh) {
#pragma unroll
                    for (int i = 0; i < W; i++) r.run[i] = 0u;
                }
            }
#pragma unroll
            for (int i = 0; i < W; i++) {
                const float t = it.s[i];
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
                        if (v.first[i] == kNoStep) v.first[i] = when;
                        v.last[i] = when;
                    }
                }
                if constexpr (EXT) {
                    if (t > x.hi[i]) { x.hi[i] = t; x.when_hi[i] = when; }
                    if (t < x.lo[i]) { x.lo[i] = t; x.when_lo[i] = when; }
                }
            }
            this->r = r;
            this->v = v;
            this->x = x;
        }
    };
};
template <bool RUNS, bool EVT, bool EXT>
__global__ __launch_bounds__(256) void k_spell_fold(const float *__restrict__ items, size_t n_pix, const SpellEntry *__restrict__ list, unsigned m, SpellAcc a)
{
    walk::lanes<SpellFold<RUNS, EVT, EXT>>(n_pix, list, m, items, a);
}
bool spell_runs(const ebcc_hip_spell_stats &st) { return st.d_run || st.d_longest || st.d_longest_end || st.d_spells || st.d_spell_steps; }
bool spell_events(const ebcc_hip_spell_stats &st) { return st.d_events || st.d_first || st.d_last; }
bool spell_extremes(const ebcc_hip_spell_stats &st) { return st.d_min || st.d_max || st.d_when_min || st.d_when_max; }
}  // namespace

void spell_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n, size_t n_pix, const uint32_t *bin, const uint32_t *when, const uint8_t *fresh,
                const ebcc_hip_spell_stats &st)
{
    const auto list = binned_list<SpellEntry>(n, bin, [&](size_t k, uint32_t b) {
        return SpellEntry{(unsigned) k, b, when ? when[k] : (unsigned) k, fresh && fresh[k] ? 1u : 0u};
    });
    if (list.empty()) return;
    const SpellAcc a{st.d_run, st.d_longest, st.d_longest_end, st.d_spells, st.d_spell_steps, st.d_events, st.d_first, st.d_last, st.d_min, st.d_max,
                     st.d_when_min, st.d_when_max, st.threshold, st.below, st.min_len};
    typedef void (*Kernel)(const float *, size_t, const SpellEntry *, unsigned, SpellAcc);
    static const Kernel kernels[8] = {nullptr, k_spell_fold<true, false, false>, k_spell_fold<false, true, false>, k_spell_fold<true, true, false>,
                                      k_spell_fold<false, false, true>, k_spell_fold<true, false, true>, k_spell_fold<false, true, true>,
                                      k_spell_fold<true, true, true>};
    const Kernel kernel = kernels[(spell_runs(st) ? 1 : 0) | (spell_events(st) ? 2 : 0) | (spell_extremes(st) ? 4 : 0)];
    walk_list(ctx, "spell_fold", list, [&](const SpellEntry *d_list, unsigned m, size_t) {
        hipLaunchKernelGGL(kernel, walk::grid(n_pix), dim3(256), 0, ctx->stream, d_items, n_pix, d_list, m, a);
    });
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
    return accumulator_bytes_checked(who, st->rows, st->cols, st->n_bins, sizeof(uint32_t));
}
long spell_stats_named(const char *who, size_t height, size_t width, const ebcc_hip_spell_stats *st, const uint32_t *bin, const uint32_t *when,
                       size_t n_steps, size_t row0, size_t col0)
{
    if (!spell_stats_shape(who, st) || !frame_window_checked(who, height, width, row0, col0, st->rows, st->cols)) return -1;
    return bins_named(who, "step", n_steps, bin, st->n_bins, [&](size_t t, uint32_t) {
        if (when ? when[t] == EBCC_HIP_NO_STEP : t >= (size_t) EBCC_HIP_NO_STEP) { set_error("%s: the label of step %zu is EBCC_HIP_NO_STEP", who, t); return false; }
        return true;
    });
}

}  // namespace ebcc
