// pair_stats.hpp - what host_codec.hip calls in pair_stats.hip: the argument check and the launcher of the pair decode
// (co-moments and vector magnitude of two variables over time per pixel; the rule is stated at ebcc_hip_pair_stats in
// include/ebcc_hip.h).
#pragma once

#include "host.hpp"

namespace ebcc {

// What ebcc_hip_pair_stats_check checks: the accumulators alone (pair_stats_shape: also what ebcc_hip_pair_stats_init needs),
// then the window in a height x width frame and the bins -> the number of named steps, or -1 with the message set.
bool pair_stats_shape(const char *who, const ebcc_hip_pair_stats *st);
long pair_stats_named(const char *who, size_t height, size_t width, const ebcc_hip_pair_stats *st, const uint32_t *bin, size_t n_steps, size_t row0,
                      size_t col0);
// The n steps that `bin` names (host, null: all bin 0; EBCC_HIP_NO_BIN: the step is not read) folded into st's accumulators, in
// index order within every bin.  The items are n_pix samples each, at any 4-byte alignment.  Step k pairs item k of d_x with
// item k of d_y (two item arrays, which may be the same one) or, `interleaved`, item 2k of d_x with item 2k + 1 of d_y (a
// decoded batch that holds x and y in turn, given as both bases).  The list goes up through the context's pinned table,
// launches of at most 65536 entries follow one another on ctx's stream, which is waited for.  st.count is the caller's.  Device
// current, the context the caller's alone, st checked (pair_stats_named).
void pair_fold(ebcc_hip_ctx *ctx, const float *d_x, const float *d_y, bool interleaved, size_t n, size_t n_pix, const uint32_t *bin,
               const ebcc_hip_pair_stats &st);

}  // namespace ebcc
