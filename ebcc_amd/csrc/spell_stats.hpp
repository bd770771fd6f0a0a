// spell_stats.hpp - what host_codec.hip calls in spell_stats.hip: the argument check and the launcher of the spell decode (run
// lengths and event timing over time per pixel; the rule is stated at ebcc_hip_spell_stats in include/ebcc_hip.h).
#pragma once

#include "host.hpp"

namespace ebcc {

// What ebcc_hip_spell_stats_check checks: the accumulators alone (spell_stats_shape: also what ebcc_hip_spell_stats_init needs),
// then the window in a height x width frame, the bins and the labels -> the number of named steps, or -1 with the message set.
bool spell_stats_shape(const char *who, const ebcc_hip_spell_stats *st);
long spell_stats_named(const char *who, size_t height, size_t width, const ebcc_hip_spell_stats *st, const uint32_t *bin, const uint32_t *when,
                       size_t n_steps, size_t row0, size_t col0);
// The n items of d_items [n][n_pix] (device, any 4-byte alignment) that `bin` names (host, null: all bin 0; EBCC_HIP_NO_BIN: the
// item is not read) folded into st's accumulators, in index order within every bin.  when (host, null: item k has label k) and
// fresh (host, null: none) are indexed as bin is.  The list goes up through the context's pinned table, launches of at most 65536
// entries follow one another on ctx's stream, which is waited for.  st.count is the caller's.  Device current, the context the
// caller's alone, st checked (spell_stats_named).
void spell_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n, size_t n_pix, const uint32_t *bin, const uint32_t *when, const uint8_t *fresh,
                const ebcc_hip_spell_stats &st);

}  // namespace ebcc
