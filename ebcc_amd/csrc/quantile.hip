// quantile.hip - the quantile decode's own part: order statistics over time at every pixel, selected on the device by a radix
// select on the order key of the samples - the check of the arguments, the workspace, the two kernels and their launchers
// (quantile.hpp).  Not in the timed encode or decode chain.  The rule is stated at ebcc_hip_time_ranks in include/ebcc_hip.h
// and restated at the kernels: that comment is the specification the tests check.
#include <climits>
#include <unordered_map>
#include "quantile.hpp"
#include "time_walk.hpp"

namespace ebcc {

// The rule.  key(x): u = bits(x + 0.0f); (u >> 31) ? ~u : u ^ 0x80000000; every NaN: 0xFFFFFFFF.  For a bin, a rank slot and
// a pixel the result is the float whose key is the rank-th smallest (0-based) of the keys of the bin's frames at that pixel.
// The select takes the key's digits of kDigitBits bits from the top: in pass s, shift = 28 - 4 s, a sample counts for a slot
// if key >> (shift + 4) == prefix (every sample in pass 0) and adds 1 to hist[(key >> shift) & 15]; the advance then takes the
// first digit d whose running total exceeds rem, rem -= (total before d), prefix = prefix << 4 | d, and zeroes the counters.
// After pass 7 prefix is the key.  Integer work throughout: no order rule is needed, and there are no atomics.
//
// k_rank_count: a lane owns one pixel - a wave reads 256 consecutive bytes of an item, and 64 consecutive counters of a digit -
// and walks the list from its first entry to its last, kDepth items in flight.  The list is grouped by bin (a stable sort on
// the host; RankEntry::run: the entries left in the bin's run, this one included), and the lane keeps the run's counters - 16
// per slot, kRankSlots slots a launch - and the slots' prefixes in registers: a digit is counted by 16 compare-and-add steps,
// every loop unrolled, so there is no LDS, no dynamic register index and no scratch.  At the end of a run the counters are
// added to the global ones [bin][slot][digit][pixel]: a batch costs one read-modify-write of the counters of each bin it
// names, not one per sample.  The private counters are 32 bits wide and a bin has fewer than 2^32 frames: none can wrap.
// Everything that decides a branch - the entry, the mask, the pass - is the same in all lanes of a workgroup.
namespace {
struct RankEntry { unsigned item, bin, mask, run; };
struct RankWork { unsigned *hist, *prefix, *rem; size_t n_pix; unsigned n_ranks; };
constexpr int kRankSlots = 4;                                       // slots a launch of k_rank_count takes: 64 counters a lane
constexpr int kDigits = 1 << kDigitBits;

__device__ inline unsigned rank_key(float x)
{
    const unsigned u = __float_as_uint(x + 0.0f);                   // (-0 -> +0)
    return x != x ? 0xFFFFFFFFu : (u >> 31) ? ~u : u ^ 0x80000000u;
}

__global__ __launch_bounds__(256) void k_rank_count(const float *__restrict__ items, RankWork w, const RankEntry *__restrict__ list, unsigned m, unsigned slot0,
                                                    int shift)
{
    constexpr int kDepth = 4;                                       // items in flight
    const size_t p = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.n_pix) return;
    const bool first_pass = shift == 32 - kDigitBits;               // (no digit above: every sample counts)
    const int above = (shift + kDigitBits) & 31;
    for (unsigned j = 0; j < m;) {
        const RankEntry head = list[j];
        const unsigned end = j + min(head.run, m - j), mask = (head.mask >> slot0) & ((1u << kRankSlots) - 1u);
        const size_t plane0 = (size_t) head.bin * w.n_ranks + slot0;
        if (!mask) { j = end; continue; }
        unsigned cnt[kRankSlots][kDigits], pre[kRankSlots];
#pragma unroll
        for (int s = 0; s < kRankSlots; s++) {
            pre[s] = 0u;
            if (!first_pass && ((mask >> s) & 1u)) pre[s] = w.prefix[(plane0 + s) * w.n_pix + p];
#pragma unroll
            for (int d = 0; d < kDigits; d++) cnt[s][d] = 0u;
        }
        for (; j < end; j += kDepth) {
            float x[kDepth];
#pragma unroll
            for (int i = 0; i < kDepth; i++)
                if (j + i < end) x[i] = items[(size_t) list[j + i].item * w.n_pix + p];
#pragma unroll
            for (int i = 0; i < kDepth; i++) {
                if (j + i >= end) break;
                const unsigned key = rank_key(x[i]), hi = first_pass ? 0u : key >> above, digit = (key >> shift) & (kDigits - 1);
#pragma unroll
                for (int s = 0; s < kRankSlots; s++) {
                    if (!((mask >> s) & 1u)) continue;
                    const unsigned dg = hi == pre[s] ? digit : (unsigned) kDigits;
#pragma unroll
                    for (int d = 0; d < kDigits; d++) cnt[s][d] += dg == (unsigned) d ? 1u : 0u;
                }
            }
        }
        j = end;
#pragma unroll
        for (int s = 0; s < kRankSlots; s++) {
            if (!((mask >> s) & 1u)) continue;
            unsigned *h = w.hist + (plane0 + s) * kDigits * w.n_pix + p;
#pragma unroll
            for (int d = 0; d < kDigits; d++) h[(size_t) d * w.n_pix] += cnt[s][d];
        }
    }
}

// One lane per (active plane, pixel): the scan of the 16 counters, the new prefix and rem, the counters zeroed for the next
// pass; `out` is given after the last pass only: the key's float, +0.0f for a zero, 0x7FC00000 for a NaN.
__global__ __launch_bounds__(256) void k_rank_advance(RankWork w, const unsigned *__restrict__ planes, float *__restrict__ out)
{
    const size_t p = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.n_pix) return;
    const size_t plane = planes[blockIdx.y], at = plane * w.n_pix + p;
    unsigned *h = w.hist + plane * kDigits * w.n_pix + p;
    unsigned c[kDigits];
#pragma unroll
    for (int d = 0; d < kDigits; d++) c[d] = h[(size_t) d * w.n_pix];
    const unsigned rem = w.rem[at];
    unsigned total = 0u, digit = 0u, before = 0u;
    bool found = false;
#pragma unroll
    for (int d = 0; d < kDigits; d++) {
        const unsigned next = total + c[d];
        if (!found && next > rem) { digit = (unsigned) d; before = total; found = true; }
        total = next;
    }
    const unsigned key = (w.prefix[at] << kDigitBits) | digit;
    w.prefix[at] = key;
    w.rem[at] = rem - before;
#pragma unroll
    for (int d = 0; d < kDigits; d++) h[(size_t) d * w.n_pix] = 0u;
    if (out) {
        const unsigned u = key == 0xFFFFFFFFu ? 0x7FC00000u : (key >> 31) ? key ^ 0x80000000u : ~key;
        out[at] = __uint_as_float(u);
    }
}
}  // namespace

void rank_begin(ebcc_hip_ctx *ctx, RankPlan &pl)
{
    const size_t planes = pl.n_bins * pl.n_ranks, work = planes * (kDigits + 2) * pl.n_pix * sizeof(unsigned);
    unsigned *base = (unsigned *) ctx->ranks.reserve(work + pl.planes.size() * sizeof(unsigned), false, false);
    pl.hist = base;
    pl.prefix = base + planes * kDigits * pl.n_pix;
    pl.rem = pl.prefix + planes * pl.n_pix;
    unsigned *table = pl.rem + planes * pl.n_pix;
    pl.d_planes = table;
    EBCC_HIP_CHECK(hipMemsetAsync(base, 0, work, ctx->stream));
    for (size_t a = 0; a < pl.planes.size(); a++)
        EBCC_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t) (pl.rem + (size_t) pl.planes[a] * pl.n_pix), (int) pl.start[a], pl.n_pix, ctx->stream));
    EBCC_HIP_CHECK(hipMemcpyAsync(table, pl.planes.data(), pl.planes.size() * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
    wait_stream(ctx->stream);
}

// Launches of at most kWalkList entries (walk_list, time_walk.hpp; a run is cut with its launch) and, within a launch, of
// kRankSlots slots each over the same items.
void rank_count(ebcc_hip_ctx *set, const RankPlan &pl, const float *d_items, size_t n, const uint32_t *bin, int pass)
{
    // (a bin none of whose slots is in use has no entries)
    auto list = binned_list<RankEntry>(n, bin, [&](size_t k, uint32_t b) { return RankEntry{(unsigned) k, b, pl.mask[b], 0u}; },
                                       [&](uint32_t b) { return pl.mask[b] != 0; });
    if (list.empty()) return;
    std::vector<unsigned> used((list.size() + kWalkList - 1) / kWalkList, 0u);     // per launch cut: the slots its bins use
    for (size_t lo = 0; lo < list.size(); lo += kWalkList)
        for (size_t e = std::min(lo + kWalkList, list.size()); e-- > lo;) {
            const bool last = e + 1 == std::min(lo + kWalkList, list.size()) || list[e + 1].bin != list[e].bin;
            list[e].run = last ? 1u : list[e + 1].run + 1u;
            used[lo / kWalkList] |= list[e].mask;
        }
    const RankWork w{pl.hist, pl.prefix, pl.rem, pl.n_pix, (unsigned) pl.n_ranks};
    walk_list(set, "rank_count", list, [&](const RankEntry *d_list, unsigned m, size_t lo) {
        for (unsigned slot0 = 0; slot0 < pl.n_ranks; slot0 += kRankSlots) {
            if (!((used[lo / kWalkList] >> slot0) & ((1u << kRankSlots) - 1u))) continue;
            hipLaunchKernelGGL(k_rank_count, dim3((unsigned) ((pl.n_pix + 255) / 256)), dim3(256), 0, set->stream, d_items, w, d_list, m, slot0,
                               32 - kDigitBits * (pass + 1));
        }
    });
}

void rank_advance(ebcc_hip_ctx *ctx, const RankPlan &pl, int pass, float *d_out)
{
    constexpr size_t kPlanes = 65535;                               // gridDim.y ends there
    const RankWork w{pl.hist, pl.prefix, pl.rem, pl.n_pix, (unsigned) pl.n_ranks};
    {
        ScopedTiming timing("rank_advance", ctx->stream);
        for (size_t lo = 0; lo < pl.planes.size(); lo += kPlanes)
            hipLaunchKernelGGL(k_rank_advance, dim3((unsigned) ((pl.n_pix + 255) / 256), (unsigned) std::min(kPlanes, pl.planes.size() - lo)), dim3(256), 0,
                               ctx->stream, w, pl.d_planes + lo, pass == kRankPasses - 1 ? d_out : nullptr);
    }
    EBCC_HIP_LAUNCH_CHECK();
    wait_stream(ctx->stream);
}

// ---- the arguments of the order statistics over time (include/ebcc_hip.h: ebcc_hip_time_ranks)
namespace {
// the spec on its face -> the bytes of the workspace, or 0 with the message set (who: may be null, then no message)
size_t time_ranks_shape(const char *who, const ebcc_hip_time_ranks *sp)
{
    auto refuse = [&](const char *what) { if (who) set_error("%s: %s", who, what); return (size_t) 0; };
    if (!sp || !sp->rank || !sp->d_out || !sp->count) return refuse("no spec, or no rank, d_out or count array");
    if (sp->n_bins < 1 || sp->rows < 1 || sp->cols < 1) return refuse("n_bins, rows and cols must not be zero");
    if (sp->n_ranks < 1 || sp->n_ranks > EBCC_HIP_MAX_RANKS) {
        if (who) set_error("%s: n_ranks is %zu, not 1 .. %d", who, sp->n_ranks, EBCC_HIP_MAX_RANKS);
        return 0;
    }
    if ((uintptr_t) sp->d_out & 3) return refuse("d_out must be 4-byte aligned");
    const size_t bytes = time_ranks_work_bytes(sp);
    if (!bytes) return refuse("the size of the output or of the workspace overflows");
    return bytes;
}
}  // namespace

// (a plane's number bin * n_ranks + slot is an unsigned on the device)
size_t time_ranks_work_bytes(const ebcc_hip_time_ranks *spec)
{
    if (!spec || spec->n_bins < 1 || spec->rows < 1 || spec->cols < 1 || spec->n_ranks < 1 || spec->n_ranks > EBCC_HIP_MAX_RANKS) return 0;
    size_t planes = 0, bytes = 0;
    if (__builtin_mul_overflow(spec->n_bins, spec->n_ranks, &planes) || planes > UINT_MAX || __builtin_mul_overflow(spec->rows, spec->cols, &bytes) ||
        __builtin_mul_overflow(bytes, planes, &bytes) || __builtin_mul_overflow(bytes, (size_t) (kDigits + 2) * sizeof(unsigned), &bytes) ||
        bytes > SIZE_MAX / 2)
        return 0;
    return bytes;
}

long time_ranks_named(const char *who, size_t height, size_t width, const ebcc_hip_time_ranks *sp, const uint32_t *bin, size_t n_frames,
                      size_t row0, size_t col0, RankPlan *plan)
{
    if (!time_ranks_shape(who, sp)) return -1;
    if (!frame_window_checked(who, height, width, row0, col0, sp->rows, sp->cols)) return -1;
    std::unordered_map<uint32_t, uint64_t> frames;                  // of the bins that are named
    const long named = bin ? bins_named(who, "frame", n_frames, bin, sp->n_bins, [&](size_t, uint32_t b) { frames[b]++; return true; })
                           : bins_named(who, "frame", n_frames, nullptr, sp->n_bins);
    if (named < 0) return -1;
    if (!bin) frames[0] = (uint64_t) named;                         // (all in bin 0: not counted one by one)
    for (const auto &bf : frames)
        if (bf.second > UINT32_MAX) { set_error("%s: bin %u is given %llu frames, not fewer than 2^32", who, bf.first, (unsigned long long) bf.second); return -1; }
    size_t used = 0;
    for (size_t b = 0; b < sp->n_bins; b++) {
        const auto it = frames.find((uint32_t) b);
        const uint64_t m = it == frames.end() ? 0 : it->second;
        for (size_t j = 0; j < sp->n_ranks; j++) {
            const size_t r = sp->rank[b * sp->n_ranks + j];
            if (r == EBCC_HIP_NO_RANK) continue;
            if (r >= m) { set_error("%s: bin %zu, slot %zu: rank %zu of %llu frames", who, b, j, r, (unsigned long long) m); return -1; }
            used++;
        }
    }
    if (!used) { set_error("%s: every rank slot is unused", who); return -1; }
    if (plan) {
        RankPlan &pl = *plan;
        pl = RankPlan{};
        pl.n_bins = sp->n_bins; pl.n_ranks = sp->n_ranks; pl.n_pix = sp->rows * sp->cols;
        pl.mask.assign(sp->n_bins, 0);
        pl.count.assign(sp->n_bins, 0);
        for (const auto &bf : frames) pl.count[bf.first] = bf.second;
        for (size_t b = 0; b < sp->n_bins; b++)
            for (size_t j = 0; j < sp->n_ranks; j++) {
                const size_t r = sp->rank[b * sp->n_ranks + j];
                if (r == EBCC_HIP_NO_RANK) continue;
                pl.mask[b] |= (uint16_t) (1u << j);
                pl.planes.push_back((unsigned) (b * sp->n_ranks + j));
                pl.start.push_back((unsigned) r);
            }
    }
    return named;
}

}  // namespace ebcc
