// time_walk.hpp - what the decodes over time share (reduce, time-map, pair, spell, and the quantile decode's list and checks):
// the walk of a lane through a list of entries on the device, the list of a batch on the host - built, grouped, sent up and
// walked in launches -, and the checks of the arguments every one of them takes.  A feature's own file keeps its rule, its
// entry, its accumulators and the state of a lane (the policy below).
#pragma once

#include <climits>
#include "host.hpp"

namespace ebcc {

// ---- device: the walk
// A lane owns pixels - a quad (4q .. 4q + 3, counted from the item's first pixel, not from an address), or one of the last
// n_pix % 4 pixels - and walks the list from its first entry to its last, kDepth entries' items in flight.  It keeps in registers
// the accumulators the current entry names, writes them back and loads others only when an entry names others; what it does
// with an entry is one lane's work in list order: no atomics, no LDS, nothing meets in a reduction tree, and everything that
// decides a branch - the entry - is the same in all lanes of a workgroup.
// The policy is a family F with F::Entry and F::Lane<W>, the state of W pixels, made from (n_pix, first pixel, the kernel's own
// arguments ..) with the start values a NULL array leaves in place:
//   Items                          what an entry loads ahead
//   load(entry, items)             the loads
//   changed(entry), held()         the entry names other accumulators than those in registers; there are some in registers
//   get(entry), put()              load the entry's accumulators (and remember which); store those in registers
//   step(entry, items)             fold (a step with conditional updates makes them on local copies of its state, as
//                                  k_spell_fold's does: on the members they compile to branches, on locals to selects)
namespace walk {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <class T> struct Vec16;                                   // the 16-byte vector of T
template <> struct Vec16<double> { typedef f64x2 type; };
template <> struct Vec16<float> { typedef f32x4 type; };
template <> struct Vec16<unsigned> { typedef u32x4 type; };
constexpr unsigned kNone = 0xFFFFFFFFu;                             // no accumulators in registers yet
constexpr int kDepth = 4;                                           // entries in flight

// W samples at p: as 16-byte accesses where W == 4 and p is on a 16-byte boundary (the same answer in every lane of a
// workgroup's quads: they lie whole quads apart), else one by one
template <class T, int W> __device__ __forceinline__ void get(const T *p, T (&r)[W])
{
    typedef typename Vec16<T>::type V;
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
template <class T, int W> __device__ __forceinline__ void put(T *p, const T (&r)[W])
{
    typedef typename Vec16<T>::type V;
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
// a lane's pixels through the list
template <class Lane> __device__ __forceinline__ void through(Lane &lane, const typename Lane::Entry *__restrict__ list, unsigned m)
{
    for (unsigned j0 = 0; j0 < m; j0 += kDepth) {
        typename Lane::Items x[kDepth];
#pragma unroll
        for (int j = 0; j < kDepth; j++)
            if (j0 + j < m) lane.load(list[j0 + j], x[j]);
#pragma unroll
        for (int j = 0; j < kDepth; j++) {
            if (j0 + j >= m) break;
            const typename Lane::Entry &e = list[j0 + j];
            if (lane.changed(e)) {
                if (lane.held()) lane.put();
                lane.get(e);
            }
            lane.step(e, x[j]);
        }
    }
    if (lane.held()) lane.put();
}
// the body of a kernel: a lane per quad of an item, then a lane per pixel of the last n_pix % 4
template <class F, class... A> __device__ __forceinline__ void lanes(size_t n_pix, const typename F::Entry *__restrict__ list, unsigned m, const A &...a)
{
    const size_t u = (size_t) blockIdx.x * blockDim.x + threadIdx.x, n4 = n_pix >> 2;
    if (u < n4) {
        typename F::template Lane<4> lane(n_pix, 4 * u, a...);
        through(lane, list, m);
    } else if (u - n4 < (n_pix & 3)) {
        typename F::template Lane<1> lane(n_pix, 4 * n4 + (u - n4), a...);
        through(lane, list, m);
    }
}
inline dim3 grid(size_t n_pix) { return dim3((unsigned) (((n_pix >> 2) + (n_pix & 3) + 255) / 256)); }
}  // namespace walk

// ---- host: the list of a batch
constexpr size_t kWalkList = 65536;                                 // entries a launch takes at the most
// The entries make(k, bin[k]) of the steps k < n that `bin` names (null: all bin 0; EBCC_HIP_NO_BIN: the step has no entry) and
// whose bin keep(bin) takes, grouped by bin: a stable sort, so within a bin still in increasing k, which is all an order rule
// fixes.
template <class Entry, class Make, class Keep> std::vector<Entry> binned_list(size_t n, const uint32_t *bin, Make make, Keep keep)
{
    std::vector<Entry> list;
    list.reserve(n);
    for (size_t k = 0; k < n; k++) {
        const uint32_t b = bin ? bin[k] : 0u;
        if (b != EBCC_HIP_NO_BIN && keep(b)) list.push_back(make(k, b));
    }
    std::stable_sort(list.begin(), list.end(), [](const Entry &p, const Entry &q) { return p.bin < q.bin; });
    return list;
}
template <class Entry, class Make> std::vector<Entry> binned_list(size_t n, const uint32_t *bin, Make make)
{
    return binned_list<Entry>(n, bin, make, [](uint32_t) { return true; });
}
// The list (not empty) goes up through the context's pinned table (boxes_reserve) and is walked under one ScopedTiming(label)
// by launch(entries on the device, their number, index of the first) - one call per cut of at most kWalkList entries, of
// [0, split) and then of [split, end), one after the other on ctx's stream, which is waited for.  A run of entries is cut with
// its launch: the next launch loads what this one stored.  Device current, the context the caller's alone.
template <class Entry, class Launch> void walk_list(ebcc_hip_ctx *ctx, const char *label, const std::vector<Entry> &list, size_t split, Launch launch)
{
    boxes_reserve(ctx, list.size(), sizeof(Entry));
    memcpy(ctx->boxes.h, list.data(), list.size() * sizeof(Entry));
    EBCC_HIP_CHECK(hipMemcpyAsync(ctx->boxes.d, ctx->boxes.h, list.size() * sizeof(Entry), hipMemcpyHostToDevice, ctx->stream));
    {
        ScopedTiming timing(label, ctx->stream);
        const size_t ends[2] = {split, list.size()};
        for (size_t lo = 0; lo < list.size();) {
            const size_t k = std::min(kWalkList, ends[lo >= split] - lo);
            launch((const Entry *) ctx->boxes.d + lo, (unsigned) k, lo);
            lo += k;
        }
    }
    EBCC_HIP_LAUNCH_CHECK();
    wait_stream(ctx->stream);
}
template <class Entry, class Launch> void walk_list(ebcc_hip_ctx *ctx, const char *label, const std::vector<Entry> &list, Launch launch)
{
    walk_list(ctx, label, list, 0, launch);
}

// ---- host: the arguments (false / -1: refused, the message set)
// a height x width frame the codec takes, and the window [row0, +rows) x [col0, +cols) inside it
inline bool frame_window_checked(const char *who, size_t height, size_t width, size_t row0, size_t col0, size_t rows, size_t cols)
{
    if (height < 1 || width < 1 || height > 2047 || width > 2047) { set_error("%s: unsupported geometry %zu x %zu", who, height, width); return false; }
    if (row0 >= height || col0 >= width || rows > height - row0 || cols > width - col0) {
        set_error("%s: the window [%zu, +%zu) x [%zu, +%zu) is not inside the %zu x %zu frame", who, row0, rows, col0, cols, height, width);
        return false;
    }
    return true;
}
// n <= most arrays of rows x cols elements of `elem` bytes
inline bool accumulator_bytes_checked(const char *who, size_t rows, size_t cols, size_t n, size_t elem, size_t most = SIZE_MAX)
{
    size_t bytes = 0;
    if (n > most || __builtin_mul_overflow(rows, cols, &bytes) || __builtin_mul_overflow(bytes, n, &bytes) || __builtin_mul_overflow(bytes, elem, &bytes)) {
        set_error("%s: the size of the accumulators overflows", who);
        return false;
    }
    return true;
}
// n of them ("frame", "step") is a number the checks can return
inline bool steps_countable(const char *who, const char *noun, size_t n)
{
    if (n > (size_t) LONG_MAX) { set_error("%s: too many %ss", who, noun); return false; }
    return true;
}
// The steps `bin` names (null: all bin 0) -> how many, each with a bin below n_bins and accepted by per_step(step, bin) (false:
// refused, its message set), and at least one.
template <class PerStep> long bins_named(const char *who, const char *noun, size_t n, const uint32_t *bin, size_t n_bins, PerStep per_step)
{
    if (!steps_countable(who, noun, n)) return -1;
    size_t named = 0;
    for (size_t t = 0; t < n; t++) {
        const uint32_t b = bin ? bin[t] : 0u;
        if (b == EBCC_HIP_NO_BIN) continue;
        if (b >= n_bins) { set_error("%s: %s %zu names bin %u of %zu", who, noun, t, b, n_bins); return -1; }
        if (!per_step(t, b)) return -1;
        named++;
    }
    if (!named) { set_error("%s: no %s is named", who, noun); return -1; }
    return (long) named;
}
inline long bins_named(const char *who, const char *noun, size_t n, const uint32_t *bin, size_t n_bins)
{
    return bins_named(who, noun, n, bin, n_bins, [](size_t, uint32_t) { return true; });
}

}  // namespace ebcc
