// array_stats.hpp - what host_codec.hip calls in array_stats.hip: launchers and argument checks of the statistics the entry
// points compute on device arrays.  Every launcher runs on the given context's stream with the device current and the context
// the caller's alone; what each computes, and in which order, is stated at its definition.
#pragma once

#include "host.hpp"

namespace ebcc {

// ---- chunk gather of the container encode
void launch_gather_chunks(const float *d_array, size_t H, size_t W, size_t ch, size_t cw, size_t first, size_t count, float *d_out, hipStream_t s);
// ---- ranges: {min key, max key, non-finite flag} per array as order keys (float_order_key), and a key's float
void group_range_keys(ebcc_hip_ctx *ctx, const float *const *ptrs, const size_t *lens, size_t n, unsigned *keys);
void host_range_keys(const float *const *ptrs, const size_t *lens, size_t n, unsigned *keys);
float float_of_order_key(uint32_t k);
int array_range(ebcc_hip_ctx *ctx, const float *d_data, size_t n, float mm[2]);
// ---- per-frame error statistics (audit, hard-bound encode)
int frame_errors(ebcc_hip_ctx *ctx, const float *d_x, const float *d_d, size_t n, size_t n_pix, const float *bound, ebcc_hip_frame_error *report);
// ---- statistics over time (reduce decode)
bool time_stats_shape(const char *who, const ebcc_hip_time_stats *st);
long time_stats_named(const char *who, size_t height, size_t width, const ebcc_hip_time_stats *st, const uint32_t *bin, size_t n_frames,
                      size_t row0, size_t col0);
void time_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n, size_t n_pix, const uint32_t *bin, const ebcc_hip_time_stats &st);
// ---- regional statistics per item (area series)
struct AreaItems { const float *d; size_t stride; unsigned pitch, row0, col0; };   // item k: d + k * stride, rows of `pitch` samples
long area_checked(const char *who, size_t height, size_t width, const ebcc_hip_area_spec *spec, ebcc_hip_region *bounding);
bool area_weights_bad(ebcc_hip_ctx *ctx, const float *d_w_pix, size_t width, const ebcc_hip_region &bb);
void area_fold(ebcc_hip_ctx *ctx, const AreaItems &items, size_t n, size_t height, size_t width, const ebcc_hip_area_spec &spec, ebcc_hip_area_stat *out);

}  // namespace ebcc
