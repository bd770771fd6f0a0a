// regrid.hpp - what host_codec.hip calls in regrid.hip: the argument check and the launcher of the regrid decode (separable
// weighted resampling of decoded frames; the arithmetic rule is stated at ebcc_hip_regrid_spec in include/ebcc_hip.h).
#pragma once

#include "host.hpp"

namespace ebcc {

// item k: d + k * stride, rows of `pitch` samples; the item is the box of its frame with the origin (row0, col0)
struct RegridItems { const float *d; size_t stride; unsigned pitch, row0, col0; };
// What ebcc_hip_regrid_check checks -> n_out_rows * n_out_cols and the box of the frame the map reads, or -1 with the message set
// and `bounding` untouched.
long regrid_checked(const char *who, size_t height, size_t width, const ebcc_hip_regrid_spec *spec, ebcc_hip_region *bounding);
// The tables of a checked spec, for items that are the box `bb` of their frames: into ctx->boxes (pinned and on the device) and
// on their way up on ctx's stream.  They stay valid until the context's next table (a context runs one call at a time).
void regrid_upload(ebcc_hip_ctx *ctx, const ebcc_hip_regrid_spec &spec, const ebcc_hip_region &bb);
// d_out [n][n_out_rows][n_out_cols] (device, any 4-byte alignment) from the n items, by the tables regrid_upload put into this
// context.  On ctx's stream, which is waited for.  Device current, the context the caller's alone.
void regrid_items(ebcc_hip_ctx *ctx, const RegridItems &items, size_t n, size_t width, const ebcc_hip_regrid_spec &spec, float *d_out);

}  // namespace ebcc
