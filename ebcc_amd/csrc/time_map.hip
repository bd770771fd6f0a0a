// time_map.hip - the time-map decode's own part: weighted sums over time at every pixel - the check of the arguments, the list
// of a batch with its groups, the kernel and its launcher (time_map.hpp).  Not in the timed encode or decode chain.  The rule
// is stated at ebcc_hip_time_map in include/ebcc_hip.h and restated at the kernel: that comment is the specification the tests
// check.
#include <climits>
#include "time_map.hpp"
#include "time_walk.hpp"

namespace ebcc {

// The rule.  For every output o and pixel p the terms of o are taken in the order of the map, which is increasing frame:
//   acc[o][p] = acc[o][p] + weight[t] * (double) x[frame[t]][p]
// the product rounded to double, then the sum rounded to double, never one FMA (-ffp-contract=off, which the whole library is
// built with).  Nothing else ever adds to an accumulator, so there are no atomics and frames never meet in a reduction tree.
//
// k_time_map is the walk of time_walk.hpp with a weight and with the group: an entry folds its item into the outputs out ..
// out + width - 1 (width <= G).  The lane keeps those outputs' accumulators in registers - G x 4 doubles, every loop unrolled, no
// dynamic register index -, writes them back and loads the next ones only when the entry names other outputs.  The host hands
// the entries of a group one after the other in increasing item (time_map_list), so a batch costs one load and one store of
// every output it names and one read of the batch per group instead of one per output.  Which lane adds a sample, and with
// which other outputs, does not matter: the additions of an (output, pixel) are one lane's, in list order.  Everything that
// decides a branch - the entry - is the same in all lanes, and no index depends on a sample: item and out come from a list the
// host has checked.  No LDS, no atomics, plain vector stores.
// Two instances: G = 1 for the entries of width 1 (4 doubles a lane), G = kMapGroup for the groups.
namespace {
template <int G> struct TimeMap {
    typedef MapEntry Entry;
    template <int W> struct Lane {
        typedef MapEntry Entry;
        struct Items { float x[W]; };
        const size_t n_pix, p0;
        const float *__restrict__ items;
        double *const acc;
        double a[G][W];
        unsigned cur = walk::kNone, wide = 0;                       // the outputs cur .. cur + wide - 1 are in registers
        __device__ __forceinline__ Lane(size_t n_pix_, size_t p0_, const float *items_, double *acc_) : n_pix(n_pix_), p0(p0_), items(items_), acc(acc_)
        {
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int i = 0; i < W; i++) a[g][i] = 0.0;
        }
        static __device__ __forceinline__ unsigned width_of(const Entry &e) { return G == 1 ? 1u : e.width; }
        __device__ __forceinline__ void load(const Entry &e, Items &it) const { walk::get<float, W>(items + (size_t) e.item * n_pix + p0, it.x); }
        __device__ __forceinline__ bool changed(const Entry &e) const { return e.out != cur || width_of(e) != wide; }
        __device__ __forceinline__ bool held() const { return cur != walk::kNone; }
        __device__ __forceinline__ void get(const Entry &e)
        {
            cur = e.out;
            wide = width_of(e);
#pragma unroll
            for (int g = 0; g < G; g++)
                if (g < (int) wide) walk::get<double, W>(acc + (size_t) (cur + g) * n_pix + p0, a[g]);
        }
        __device__ __forceinline__ void put()
        {
#pragma unroll
            for (int g = 0; g < G; g++)
                if (g < (int) wide) walk::put<double, W>(acc + (size_t) (cur + g) * n_pix + p0, a[g]);
        }
        __device__ __forceinline__ void step(const Entry &e, const Items &it)
        {
            const unsigned wd = width_of(e);
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (g >= (int) wd) break;
                const double wt = e.w[g];
#pragma unroll
                for (int i = 0; i < W; i++) {
                    const double t = wt * (double) it.x[i];         // rounded to double
                    a[g][i] = a[g][i] + t;                          // rounded to double: two roundings, never an FMA
                }
            }
        }
    };
};
template <int G>
__global__ __launch_bounds__(256) void k_time_map(const float *__restrict__ items, size_t n_pix, const MapEntry *__restrict__ list, unsigned m, double *acc)
{
    walk::lanes<TimeMap<G>>(n_pix, list, m, items, acc);
}
}  // namespace

void time_map_list(const ebcc_hip_time_map &map, size_t f_lo, size_t f_hi, const uint32_t *slot, size_t base, std::vector<MapEntry> &list)
{
    // every output's terms inside the range: frames increase within an output
    std::vector<std::pair<size_t, size_t>> span(map.n_out);
    for (size_t o = 0; o < map.n_out; o++) {
        const uint32_t *lo = map.frame + map.start[o], *hi = map.frame + map.start[o + 1];
        const uint32_t *a = std::lower_bound(lo, hi, f_lo, [](uint32_t f, size_t v) { return (size_t) f < v; });
        const uint32_t *b = std::lower_bound(a, hi, f_hi, [](uint32_t f, size_t v) { return (size_t) f < v; });
        span[o] = {(size_t) (a - map.frame), (size_t) (b - map.frame)};
    }
    for (size_t o = 0; o < map.n_out;) {
        const size_t a = span[o].first, n = span[o].second - a;
        if (!n) { o++; continue; }
        size_t wd = 1;
        while (wd < (size_t) kMapGroup && o + wd < map.n_out && span[o + wd].second - span[o + wd].first == n &&
               !memcmp(map.frame + span[o + wd].first, map.frame + a, n * sizeof(uint32_t))) wd++;
        for (size_t t = 0; t < n; t++) {
            const size_t f = map.frame[a + t];
            MapEntry e{(unsigned) ((slot ? slot[f] : f) - base), (unsigned) o, (unsigned) wd, 0u, {0.0, 0.0, 0.0, 0.0}};
            for (size_t g = 0; g < wd; g++) e.w[g] = map.weight[span[o + g].first + t];
            list.push_back(e);
        }
        o += wd;
    }
}

void time_map(ebcc_hip_ctx *ctx, const float *d_items, size_t n_pix, const ebcc_hip_time_map &map, size_t f_lo, size_t f_hi, const uint32_t *slot,
              size_t base)
{
    std::vector<MapEntry> list;
    time_map_list(map, f_lo, f_hi, slot, base, list);
    if (list.empty()) return;
    // the entries of width 1 first: they run in the instance that keeps one output's accumulators
    const size_t n_one = (size_t) (std::stable_partition(list.begin(), list.end(), [](const MapEntry &e) { return e.width == 1; }) - list.begin());
    walk_list(ctx, "time_map", list, n_one, [&](const MapEntry *d_list, unsigned m, size_t lo) {
        hipLaunchKernelGGL(lo < n_one ? k_time_map<1> : k_time_map<kMapGroup>, walk::grid(n_pix), dim3(256), 0, ctx->stream, d_items, n_pix, d_list, m, map.d_acc);
    });
}

// ---- the arguments of the weighted sums over time (include/ebcc_hip.h: ebcc_hip_time_map)
long time_map_named(const char *who, size_t height, size_t width, const ebcc_hip_time_map *map, size_t n_frames, size_t row0, size_t col0,
                    std::vector<uint32_t> *named)
{
    if (!map || !map->start || !map->d_acc || !map->count) { set_error("%s: no map, or no start, d_acc or count array", who); return -1; }
    if (map->n_out < 1 || map->rows < 1 || map->cols < 1) { set_error("%s: n_out, rows and cols must not be zero", who); return -1; }
    if ((uintptr_t) map->d_acc & 7) { set_error("%s: d_acc must be 8-byte aligned", who); return -1; }
    if (!accumulator_bytes_checked(who, map->rows, map->cols, map->n_out, sizeof(double), 0xFFFFFFFEu) ||       // (out + width is an unsigned)
        !frame_window_checked(who, height, width, row0, col0, map->rows, map->cols) || !steps_countable(who, "frame", n_frames)) return -1;
    if (map->start[0] != 0) { set_error("%s: start[0] must be 0", who); return -1; }
    for (size_t o = 0; o < map->n_out; o++)
        if (map->start[o + 1] < map->start[o]) { set_error("%s: start decreases at output %zu", who, o); return -1; }
    const size_t n_terms = map->start[map->n_out];
    if (!n_terms) { set_error("%s: no term at all", who); return -1; }
    if (!map->frame || !map->weight) { set_error("%s: no frame or no weight array", who); return -1; }
    for (size_t o = 0; o < map->n_out; o++)
        for (size_t t = map->start[o]; t < map->start[o + 1]; t++) {
            if (map->frame[t] >= n_frames) { set_error("%s: term %zu of output %zu names frame %u of %zu", who, t - map->start[o], o, map->frame[t], n_frames); return -1; }
            if (t > map->start[o] && map->frame[t] <= map->frame[t - 1]) {
                set_error("%s: the frames of output %zu are not strictly increasing at term %zu", who, o, t - map->start[o]);
                return -1;
            }
            if (!std::isfinite(map->weight[t])) { set_error("%s: the weight of term %zu of output %zu is not finite", who, t - map->start[o], o); return -1; }
        }
    // the distinct frames: marked in a table where the frame axis is not much longer than the list, else sorted
    std::vector<uint32_t> seen;
    if (n_frames / 8 <= n_terms + 65536) {
        std::vector<uint8_t> mark(n_frames, 0);
        for (size_t t = 0; t < n_terms; t++) mark[map->frame[t]] = 1;
        for (size_t f = 0; f < n_frames; f++)
            if (mark[f]) seen.push_back((uint32_t) f);
    } else {
        seen.assign(map->frame, map->frame + n_terms);
        std::sort(seen.begin(), seen.end());
        seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    }
    const long n = (long) seen.size();
    if (named) named->swap(seen);
    return n;
}

}  // namespace ebcc
