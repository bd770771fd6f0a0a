// time_map.hip - the time-map decode's own part: weighted sums over time at every pixel - the check of the arguments, the list
// of a batch with its groups, the kernel and its launcher (time_map.hpp).  Not in the timed encode or decode chain.  The rule
// is stated at ebcc_hip_time_map in include/ebcc_hip.h and restated at the kernel: that comment is the specification the tests
// check.
#include <climits>
#include "time_map.hpp"

namespace ebcc {

// The rule.  For every output o and pixel p the terms of o are taken in the order of the map, which is increasing frame:
//   acc[o][p] = acc[o][p] + weight[t] * (double) x[frame[t]][p]
// the product rounded to double, then the sum rounded to double, never one FMA (-ffp-contract=off, which the whole library is
// built with).  Nothing else ever adds to an accumulator, so there are no atomics and frames never meet in a reduction tree.
//
// k_time_map is k_time_fold (array_stats.hip) with a weight and with the group: a lane owns a quad of pixels (4q .. 4q + 3,
// counted from the item's first pixel; the last n_pix % 4 pixels go one to a lane) and walks the list from its first entry to
// its last, four items in flight - one 16-byte load from an item that begins on a 16-byte boundary, four 4-byte loads from one
// that does not.  An entry folds its item into the outputs out .. out + width - 1 (width <= G): the lane keeps those outputs'
// accumulators in registers - G x 4 doubles, every loop unrolled, no dynamic register index -, writes them back and loads the
// next ones only when the entry names other outputs.  The host hands the entries of a group one after the other in increasing
// item (time_map_list), so a batch costs one load and one store of every output it names and one read of the batch per group
// instead of one per output.  Which lane adds a sample, and with which other outputs, does not matter: the additions of an
// (output, pixel) are one lane's, in list order.  Everything that decides a branch - the entry - is the same in all lanes, and
// no index depends on a sample: item and out come from a list the host has checked.  No LDS, no atomics, plain vector stores.
// Two instances: G = 1 for the entries of width 1 (4 doubles a lane), G = kMapGroup for the groups.
namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// W floats at p: one 16-byte load where W == 4 and p is on a 16-byte boundary (the same answer in every lane of a
// workgroup's quads: they lie whole quads apart), else one by one
template <int W> __device__ inline void map_get(const float *p, float (&r)[W])
{
    if constexpr (W == 4) {
        if (((uintptr_t) p & 15) == 0) {
            const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
            for (int i = 0; i < 4; i++) r[i] = q[i];
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) r[i] = p[i];
}
// W doubles at p (8-byte aligned): as 16-byte accesses where W == 4 and p is on a 16-byte boundary
template <int W> __device__ inline void map_get(const double *p, double (&r)[W])
{
    if constexpr (W == 4) {
        if (((uintptr_t) p & 15) == 0) {
#pragma unroll
            for (int v = 0; v < 2; v++) {
                const f64x2 q = reinterpret_cast<const f64x2 *>(p)[v];
                r[2 * v] = q[0];
                r[2 * v + 1] = q[1];
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) r[i] = p[i];
}
template <int W> __device__ inline void map_put(double *p, const double (&r)[W])
{
    if constexpr (W == 4) {
        if (((uintptr_t) p & 15) == 0) {
#pragma unroll
            for (int v = 0; v < 2; v++) {
                f64x2 q;
                q[0] = r[2 * v];
                q[1] = r[2 * v + 1];
                reinterpret_cast<f64x2 *>(p)[v] = q;
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) p[i] = r[i];
}

// the pixels p0 .. p0 + W - 1 through the list
template <int G, int W>
__device__ inline void time_map_pixels(const float *__restrict__ items, size_t n_pix, size_t p0, const MapEntry *__restrict__ list, unsigned m, double *acc)
{
    constexpr unsigned kNone = 0xFFFFFFFFu;
    constexpr int kDepth = 4;                                       // items in flight
    double a[G][W];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int i = 0; i < W; i++) a[g][i] = 0.0;
    unsigned cur = kNone, wide = 0;                                 // the outputs cur .. cur + wide - 1 are in registers
    auto get = [&]() {
#pragma unroll
        for (int g = 0; g < G; g++)
            if (g < (int) wide) map_get<W>(acc + (size_t) (cur + g) * n_pix + p0, a[g]);
    };
    auto put = [&]() {
#pragma unroll
        for (int g = 0; g < G; g++)
            if (g < (int) wide) map_put<W>(acc + (size_t) (cur + g) * n_pix + p0, a[g]);
    };
    for (unsigned j0 = 0; j0 < m; j0 += kDepth) {
        float x[kDepth][W];
#pragma unroll
        for (int j = 0; j < kDepth; j++)
            if (j0 + j < m) map_get<W>(items + (size_t) list[j0 + j].item * n_pix + p0, x[j]);
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            if (j0 + j >= m) break;
            const MapEntry &e = list[j0 + j];
            const unsigned o = e.out, wd = G == 1 ? 1u : e.width;
            if (o != cur || wd != wide) {
                if (cur != kNone) put();
                cur = o;
                wide = wd;
                get();
            }
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (g >= (int) wd) break;
                const double wt = e.w[g];
#pragma unroll
                for (int i = 0; i < W; i++) {
                    const double t = wt * (double) x[j][i];         // rounded to double
                    a[g][i] = a[g][i] + t;                          // rounded to double: two roundings, never an FMA
                }
            }
        }
    }
    if (cur != kNone) put();
}
// a lane per quad of an item, then a lane per pixel of the last n_pix % 4
template <int G>
__global__ __launch_bounds__(256) void k_time_map(const float *__restrict__ items, size_t n_pix, const MapEntry *__restrict__ list, unsigned m, double *acc)
{
    const size_t u = (size_t) blockIdx.x * blockDim.x + threadIdx.x, n4 = n_pix >> 2;
    if (u < n4) time_map_pixels<G, 4>(items, n_pix, 4 * u, list, m, acc);
    else if (u - n4 < (n_pix & 3)) time_map_pixels<G, 1>(items, n_pix, 4 * n4 + (u - n4), list, m, acc);
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
    constexpr size_t kList = 65536;
    std::vector<MapEntry> list;
    time_map_list(map, f_lo, f_hi, slot, base, list);
    if (list.empty()) return;
    // the entries of width 1 first: they run in the instance that keeps one output's accumulators
    const size_t n_one = (size_t) (std::stable_partition(list.begin(), list.end(), [](const MapEntry &e) { return e.width == 1; }) - list.begin());
    boxes_reserve(ctx, list.size(), sizeof(MapEntry));
    memcpy(ctx->boxes.h, list.data(), list.size() * sizeof(MapEntry));
    EBCC_HIP_CHECK(hipMemcpyAsync(ctx->boxes.d, ctx->boxes.h, list.size() * sizeof(MapEntry), hipMemcpyHostToDevice, ctx->stream));
    const MapEntry *d_list = (const MapEntry *) ctx->boxes.d;
    const size_t lanes = (n_pix >> 2) + (n_pix & 3);
    const dim3 grid((unsigned) ((lanes + 255) / 256));
    {
        ScopedTiming timing("time_map", ctx->stream);
        // a run of entries is cut with its launch: the next launch loads what this one stored
        for (size_t lo = 0; lo < n_one; lo += kList)
            hipLaunchKernelGGL(k_time_map<1>, grid, dim3(256), 0, ctx->stream, d_items, n_pix, d_list + lo, (unsigned) std::min(kList, n_one - lo), map.d_acc);
        for (size_t lo = n_one; lo < list.size(); lo += kList)
            hipLaunchKernelGGL(k_time_map<kMapGroup>, grid, dim3(256), 0, ctx->stream, d_items, n_pix, d_list + lo,
                               (unsigned) std::min(kList, list.size() - lo), map.d_acc);
    }
    EBCC_HIP_LAUNCH_CHECK();
    wait_stream(ctx->stream);
}

// ---- the arguments of the weighted sums over time (include/ebcc_hip.h: ebcc_hip_time_map)
long time_map_named(const char *who, size_t height, size_t width, const ebcc_hip_time_map *map, size_t n_frames, size_t row0, size_t col0,
                    std::vector<uint32_t> *named)
{
    if (!map || !map->start || !map->d_acc || !map->count) { set_error("%s: no map, or no start, d_acc or count array", who); return -1; }
    if (map->n_out < 1 || map->rows < 1 || map->cols < 1) { set_error("%s: n_out, rows and cols must not be zero", who); return -1; }
    if ((uintptr_t) map->d_acc & 7) { set_error("%s: d_acc must be 8-byte aligned", who); return -1; }
    size_t bytes = 0;
    if (map->n_out >= 0xFFFFFFFFu || __builtin_mul_overflow(map->rows, map->cols, &bytes) || __builtin_mul_overflow(bytes, map->n_out, &bytes) ||
        __builtin_mul_overflow(bytes, sizeof(double), &bytes)) { set_error("%s: the size of the accumulators overflows", who); return -1; }
    if (height < 1 || width < 1 || height > 2047 || width > 2047) { set_error("%s: unsupported geometry %zu x %zu", who, height, width); return -1; }
    if (row0 >= height || col0 >= width || map->rows > height - row0 || map->cols > width - col0) {
        set_error("%s: the window [%zu, +%zu) x [%zu, +%zu) is not inside the %zu x %zu frame", who, row0, map->rows, col0, map->cols, height, width);
        return -1;
    }
    if (n_frames > (size_t) LONG_MAX) { set_error("%s: too many frames", who); return -1; }
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
