// time_map.hpp - what host_codec.hip calls in time_map.hip: the argument check, the list of a batch and the launcher of the
// time-map decode (weighted sums over time per pixel: acc[o] = acc[o] + weight * x, terms in increasing frame; the rule is stated
// at ebcc_hip_time_map in include/ebcc_hip.h).
#pragma once

#include "host.hpp"

namespace ebcc {

constexpr int kMapGroup = 4;                                // outputs a list entry folds one loaded item into, at the most
// One step of a lane's walk: item `item` of the batch is folded into the outputs out .. out + width - 1 with their weights.
struct MapEntry { unsigned item, out, width, pad; double w[kMapGroup]; };
static_assert(sizeof(MapEntry) == 48, "one entry is 48 bytes");

// What ebcc_hip_time_map_check checks -> the number of distinct frames named, or -1 with the message set.  named: filled for a
// call that is accepted with those frames in increasing order (the check alone allocates nothing that outlives it).
long time_map_named(const char *who, size_t height, size_t width, const ebcc_hip_time_map *map, size_t n_frames, size_t row0, size_t col0,
                    std::vector<uint32_t> *named = nullptr);
// Host only: the entries of the terms of a checked map whose frame lies in [f_lo, f_hi), appended to `list`.  The item of a frame
// f is slot[f] - base (slot null: f - base).  Consecutive outputs whose terms in the range name the same frames form a group of
// up to kMapGroup outputs; a group's entries follow one another in increasing frame, the groups in increasing output: for every
// (output, pixel) the terms stay in the order of the map.
void time_map_list(const ebcc_hip_time_map &map, size_t f_lo, size_t f_hi, const uint32_t *slot, size_t base, std::vector<MapEntry> &list);
// The terms of `map` with a frame in [f_lo, f_hi) folded from d_items [.][n_pix] (device, any 4-byte alignment; item of a frame
// as in time_map_list) into map.d_acc.  The list goes up through the context's pinned table, launches of at most 65536 entries
// follow one another on ctx's stream, which is waited for.  map.count is the caller's.  Device current, the context the
// caller's alone, map checked (time_map_named).
void time_map(ebcc_hip_ctx *ctx, const float *d_items, size_t n_pix, const ebcc_hip_time_map &map, size_t f_lo, size_t f_hi, const uint32_t *slot,
              size_t base);

}  // namespace ebcc
