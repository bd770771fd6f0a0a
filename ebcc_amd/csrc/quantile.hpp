// quantile.hpp - what host_codec.hip calls in quantile.hip: the argument check, the workspace and the two launchers of the
// quantile decode (order statistics over time per pixel by a radix select on the order key; the rule is stated at
// ebcc_hip_time_ranks in include/ebcc_hip.h).
#pragma once

#include "host.hpp"

namespace ebcc {

constexpr int kDigitBits = 4;                               // digit of the radix select
constexpr int kRankPasses = 32 / kDigitBits;                // passes over the series, most significant digit first

// A checked call, as the launchers need it: the planes [bin][slot] that are in use, each bin's slots as a mask, each bin's
// frames, and - once rank_begin has run - where the workspace lies.
struct RankPlan {
    size_t n_bins = 0, n_ranks = 0, n_pix = 0;
    std::vector<unsigned> planes, start;                    // active planes (bin * n_ranks + slot) in increasing order, and their ranks
    std::vector<uint16_t> mask;                             // [n_bins]: bit j: slot j is in use
    std::vector<uint64_t> count;                            // [n_bins]: frames named
    unsigned *hist = nullptr, *prefix = nullptr, *rem = nullptr;      // device: [planes][16][n_pix], [planes][n_pix] twice
    const unsigned *d_planes = nullptr;                     // device: `planes`
};
// What ebcc_hip_time_ranks_check checks -> the number of named frames, or -1 with the message set.  plan: filled for a call
// that is accepted (the check alone allocates nothing that grows with n_bins).
long time_ranks_named(const char *who, size_t height, size_t width, const ebcc_hip_time_ranks *spec, const uint32_t *bin, size_t n_frames,
                      size_t row0, size_t col0, RankPlan *plan = nullptr);
// (16 + 2) * 4 bytes per (bin, slot, pixel); 0: overflow or a spec the check refuses on its face
size_t time_ranks_work_bytes(const ebcc_hip_time_ranks *spec);
// The workspace in ctx->ranks (grown on demand; throws HipFailure without memory) and its start values: prefix 0, rem the
// rank, counters 0.  On ctx's stream, which is waited for.  Device current, the context the caller's alone.
void rank_begin(ebcc_hip_ctx *ctx, RankPlan &plan);
// Pass `pass` over the items d_items [n][n_pix] (device, any 4-byte alignment) that `bin` names: their digits counted into the
// plan's counters.  The list goes up through set's pinned table, the launches run on set's stream, which is waited for: set may
// be either engine set of the context whose workspace the plan names, one at a time.
void rank_count(ebcc_hip_ctx *set, const RankPlan &plan, const float *d_items, size_t n, const uint32_t *bin, int pass);
// After every batch of pass `pass` is counted: each active (bin, slot, pixel) takes its digit, and after the last pass writes
// its float to d_out [n_bins][n_ranks][n_pix].  On ctx's stream, which is waited for.
void rank_advance(ebcc_hip_ctx *ctx, const RankPlan &plan, int pass, float *d_out);

}  // namespace ebcc
