// regrid.hip - the regrid decode's own part: decoded frames (or boxes of them) resampled by a separable linear map with a
// contiguous support per output position - the check of the map, its tables, the kernel and its launcher (regrid.hpp).  Not in
// the timed encode or decode chain.  The arithmetic rule is stated at ebcc_hip_regrid_spec in include/ebcc_hip.h and restated
// at the kernel: that comment is the specification the tests check.
#include <climits>
#include <cmath>
#include "regrid.hpp"

namespace ebcc {

// The rule, for output (R, C) of an item with samples x:
//   a = +0.0;  for i = 0 .. rows.count[R), increasing:  r = rows.first[R] + i
//       t = +0.0;  for j = 0 .. cols.count[C), increasing:  t = t + (double) x[r][col(C, j)] * wc[C][j]
//       a = a + wr[R][i] * t
//   out[R][C] = (float) a
// col(C, j) = cols.first[C] + j, taken % width when the column map wraps.  The fused form: one workgroup per (item, output row,
// run of 256 output columns), one thread per output column, which recomputes t for every output row whose support holds the row
// r - t depends on (r, C) alone, so the bits are those of a two-pass form.  The loop over the support rows is uniform over the
// workgroup (its bounds and the row weights come from blockIdx: scalar loads); each thread reads its own count[C] consecutive
// samples of a row, so the loads of neighbouring lanes are neighbouring runs.  No LDS, no atomics, 4-byte loads and stores:
// items and output may lie at any 4-byte alignment.  kShort: every column support has at most kShortTaps taps (and the
// frame at least as many columns, where the map wraps) - the column weights (+0.0 past the support) and the columns are
// read once into registers and a row's samples are loaded together (0 past the support: such a term is +0.0 and changes
// no t, which starts at +0.0 and so never is -0.0).
namespace {
struct RegridTap { unsigned first, count, off; };                       // first: within the item; off: of the first weight
struct RegridTables { const double *wr, *wc; const RegridTap *rows, *cols; unsigned n_out_rows, n_out_cols, width, wrap; };
constexpr int kShortTaps = 8;
template <bool kShort>
__global__ __launch_bounds__(256) void k_regrid(RegridItems items, RegridTables tb, float *__restrict__ out)
{
    const unsigned C = blockIdx.x * 256u + threadIdx.x, R = blockIdx.y, item = blockIdx.z;
    if (C >= tb.n_out_cols) return;
    const RegridTap row = tb.rows[R], col = tb.cols[C];
    const double *__restrict__ wr = tb.wr + row.off, *__restrict__ wc = tb.wc + col.off;
    const float *__restrict__ x = items.d + (size_t) item * items.stride + (size_t) row.first * items.pitch;
    double a = 0.0;
    if constexpr (kShort) {
        double w[kShortTaps];
#pragma unroll
        for (int j = 0; j < kShortTaps; j++) w[j] = (unsigned) j < col.count ? wc[j] : 0.0;
        unsigned at[kShortTaps];                                        // (first + j < 2 * width: one subtraction is the % width)
#pragma unroll
        for (int j = 0; j < kShortTaps; j++) at[j] = tb.wrap && col.first + j >= tb.width ? col.first + j - tb.width : col.first + j;
        for (unsigned i = 0; i < row.count; i++, x += items.pitch) {
            float v[kShortTaps];
#pragma unroll
            for (int j = 0; j < kShortTaps; j++) v[j] = (unsigned) j < col.count ? x[at[j]] : 0.0f;
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < kShortTaps; j++) t = t + (double) v[j] * w[j];
            a = a + wr[i] * t;
        }
    } else {
        for (unsigned i = 0; i < row.count; i++, x += items.pitch) {
            double t = 0.0;
            if (tb.wrap)
                for (unsigned j = 0; j < col.count; j++) t = t + (double) x[(col.first + j) % tb.width] * wc[j];
            else
                for (unsigned j = 0; j < col.count; j++) t = t + (double) x[col.first + j] * wc[j];
            a = a + wr[i] * t;
        }
    }
    out[((size_t) item * tb.n_out_rows + R) * tb.n_out_cols + C] = (float) a;
}

// one axis of a spec: refusals -> false with the message set; else the source range [lo, hi) its supports read
bool axis_checked(const char *who, const char *axis, const ebcc_hip_axis_map &m, size_t extent, bool may_wrap, size_t *lo, size_t *hi, size_t *taps)
{
    if (!m.first || !m.count || !m.weight) { set_error("%s: the %s map lacks a table", who, axis); return false; }
    if (m.n_out < 1 || m.n_out > 65535) { set_error("%s: the %s map has %zu outputs, 1 .. 65535 are supported", who, axis, m.n_out); return false; }
    if (m.wrap && !may_wrap) { set_error("%s: only the column map may wrap", who); return false; }
    size_t a = extent, b = 0, total = 0;
    for (size_t i = 0; i < m.n_out; i++) {
        const size_t f = m.first[i], c = m.count[i];
        if (c < 1 || c > EBCC_HIP_REGRID_MAX_TAPS) {
            set_error("%s: %s output %zu has %zu taps, 1 .. %d are supported", who, axis, i, c, EBCC_HIP_REGRID_MAX_TAPS);
            return false;
        }
        if (f >= extent) { set_error("%s: %s output %zu begins at %zu, outside the extent %zu", who, axis, i, f, extent); return false; }
        if (c > extent - f) {
            if (!m.wrap) { set_error("%s: the support [%zu, +%zu) of %s output %zu leaves the extent %zu", who, f, c, axis, i, extent); return false; }
            a = 0; b = extent;
        }
        a = std::min(a, f); b = std::max(b, std::min(f + c, extent));
        for (size_t j = 0; j < c; j++)
            if (!std::isfinite(m.weight[total + j])) { set_error("%s: weight %zu of %s output %zu is a NaN or an Inf", who, j, axis, i); return false; }
        total += c;
    }
    *lo = a; *hi = b; *taps = total;
    return true;
}
}  // namespace

long regrid_checked(const char *who, size_t height, size_t width, const ebcc_hip_regrid_spec *spec, ebcc_hip_region *bounding)
{
    if (!spec) { set_error("%s: no spec", who); return -1; }
    if (height < 1 || width < 1 || height > 2047 || width > 2047) { set_error("%s: unsupported geometry %zu x %zu", who, height, width); return -1; }
    size_t r0, r1, c0, c1, tr, tc;
    if (!axis_checked(who, "row", spec->rows, height, false, &r0, &r1, &tr) || !axis_checked(who, "column", spec->cols, width, true, &c0, &c1, &tc)) return -1;
    size_t bytes = 0;
    const size_t n = spec->rows.n_out * spec->cols.n_out;               // (at most 65535^2)
    if (n > (size_t) LONG_MAX / sizeof(float) || __builtin_mul_overflow(n, sizeof(float), &bytes)) { set_error("%s: the size of the output overflows", who); return -1; }
    if (bounding) *bounding = ebcc_hip_region{r0, c0, r1 - r0, c1 - c0};
    return (long) n;
}

void regrid_upload(ebcc_hip_ctx *ctx, const ebcc_hip_regrid_spec &spec, const ebcc_hip_region &bb)
{
    const ebcc_hip_axis_map *const axis[2] = {&spec.rows, &spec.cols};
    const size_t origin[2] = {bb.row0, bb.col0};
    size_t taps[2] = {0, 0};
    for (int k = 0; k < 2; k++) for (size_t i = 0; i < axis[k]->n_out; i++) taps[k] += axis[k]->count[i];
    const size_t w_bytes = (taps[0] + taps[1]) * sizeof(double), bytes = w_bytes + (spec.rows.n_out + spec.cols.n_out) * sizeof(RegridTap);
    boxes_reserve(ctx, 1, bytes);
    double *w = (double *) ctx->boxes.h;
    RegridTap *tap = (RegridTap *) ((char *) ctx->boxes.h + w_bytes);
    for (int k = 0; k < 2; k++) {
        memcpy(w, axis[k]->weight, taps[k] * sizeof(double));
        size_t off = 0;
        for (size_t i = 0; i < axis[k]->n_out; i++) {
            tap[i] = RegridTap{(unsigned) (axis[k]->first[i] - origin[k]), axis[k]->count[i], (unsigned) off};
            off += axis[k]->count[i];
        }
        w += taps[k]; tap += axis[k]->n_out;
    }
    EBCC_HIP_CHECK(hipMemcpyAsync(ctx->boxes.d, ctx->boxes.h, bytes, hipMemcpyHostToDevice, ctx->stream));
}

// Items per launch: the item is blockIdx.z, and gridDim.z ends at 65535.  (gridDim.y is the output row, at most 65535 by the
// check; gridDim.x the runs of 256 output columns, at most 256.)
constexpr size_t kRegridItems = 65535;
void regrid_items(ebcc_hip_ctx *ctx, const RegridItems &items, size_t n, size_t width, const ebcc_hip_regrid_spec &spec, float *d_out)
{
    const size_t Ro = spec.rows.n_out, Co = spec.cols.n_out;
    size_t tr = 0, tc = 0;
    uint32_t longest = 0;
    for (size_t i = 0; i < Ro; i++) tr += spec.rows.count[i];
    for (size_t i = 0; i < Co; i++) { tc += spec.cols.count[i]; longest = std::max(longest, spec.cols.count[i]); }
    const double *d_w = (const double *) ctx->boxes.d;
    const RegridTap *d_tap = (const RegridTap *) ((const char *) ctx->boxes.d + (tr + tc) * sizeof(double));
    const RegridTables tb{d_w, d_w + tr, d_tap, d_tap + Ro, (unsigned) Ro, (unsigned) Co, (unsigned) width, spec.cols.wrap ? 1u : 0u};
    const bool brief = longest <= (uint32_t) kShortTaps && (!spec.cols.wrap || width >= (size_t) kShortTaps);
    {
        ScopedTiming timing("regrid", ctx->stream);
        for (size_t lo = 0; lo < n; lo += kRegridItems) {
            const size_t m = std::min(kRegridItems, n - lo);
            RegridItems part = items;
            part.d += lo * items.stride;
            const dim3 grid((unsigned) ((Co + 255) / 256), (unsigned) Ro, (unsigned) m);
            float *const o = d_out + lo * Ro * Co;
            if (brief) hipLaunchKernelGGL(k_regrid<true>, grid, dim3(256), 0, ctx->stream, part, tb, o);
            else hipLaunchKernelGGL(k_regrid<false>, grid, dim3(256), 0, ctx->stream, part, tb, o);
        }
    }
    EBCC_HIP_LAUNCH_CHECK();
    wait_stream(ctx->stream);
}

}  // namespace ebcc
