/*
 * ebcc_hip.h - C-ABI of the MI355X (gfx950) EBCC engine: plain pointers and sizes only.
 *
 * The drop-in surface of the reference is include/ebcc_codec.h (same symbols as
 * /root/reference/src/ebcc_codec.h:41-49 plus the HDF5 plugin symbols of src/h5z_ebcc.c:14-28,38).
 * This header is ADDITIVE: device-resident batch entry points that the reference cannot offer
 * (its API is one host frame per call), plus unit-level entry points used by the parity tests.
 * Every function cites the reference interface it replaces.
 *
 * Conventions: return 0 on success, non-zero on error (message on stderr); "d_" pointers are HIP
 * device pointers on the context's device; all other pointers are host memory; work is enqueued on
 * the context's stream and the call returns after the stream has been synchronised unless stated.
 *
 * Caller buffers: device and host frame pointers (d_frames, d_images, d_out, h_frames, ...) need 4-byte alignment only - a
 * frame inside a larger tensor is passed as it lies.  Exactly [n_frames][height][width] floats are read from an input (it
 * is never written) or written to an output: nothing in front of it, behind it, or behind frame n_frames of a partial
 * batch is touched, also by a call that fails.  Results do not depend on the alignment; the kernels use wider accesses
 * where base and frame size allow them, and a decode output on a 256-byte boundary is written directly instead of through
 * one device-to-device copy of the batch.  (tests/test_caller_buffers_gpu.py)
 *
 * Threads: every entry point that codes, decodes, audits, reduces, folds or selects on a context (ebcc_hip_quantile_shard and
 * ebcc_hip_rank_items among them: each holds the lock from its first pass to its last) - and ebcc_hip_upload, _download,
 * _prepare and _release_second_set - takes the lock of the context's device for the call, as the entry points of
 * include/ebcc_codec.h do for the engines they cache per (device, frame geometry); ebcc_hip_release_engines takes it device by
 * device.  Calls on one device run one after the other, so threads may share a context, each with buffers of its own; calls on
 * different devices do not wait for each other.  NOT serialised: ebcc_hip_create / _destroy and ebcc_hip_malloc / _free /
 * _memcpy_h2d / _memcpy_d2h - safe beside any running call, and they leave the calling thread's current device as it was -, the
 * unit hooks ebcc_hip_spiht_*, ebcc_hip_residual_* and ebcc_hip_j2k_* - their context must not be in use by another thread - and
 * ebcc_hip_timing_enable / _timing_read.  Destroying a context while a call on it is running or waiting is the caller's error.
 * ebcc_hip_last_error is per thread.  (tests/test_threads_gpu.py)
 */
#ifndef EBCC_HIP_H
#define EBCC_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "ebcc_codec.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct ebcc_hip_ctx ebcc_hip_ctx;

/* ---- context -------------------------------------------------------------------------------- */
int ebcc_hip_device_count(void);
/* One context per (device, frame geometry); owns a HIP stream and all workspaces for up to
 * max_frames frames of height x width.  Returns NULL on failure.
 * max_frames is at most EBCC_HIP_MAX_FRAMES: the batch kernels take the frame from blockIdx.y, whose range ends there.  A
 * larger context is refused with a message (ebcc_hip_last_error) before anything is allocated; larger arrays go through the
 * shard and host-frames entry points, which run batches of the context's capacity.  (For the chunks of several frames of the
 * reference-compatible entry points the limit is on frames times tiles; EBCC_HIP_MAX_BATCH is capped accordingly.) */
#define EBCC_HIP_MAX_FRAMES 65535
ebcc_hip_ctx *ebcc_hip_create(int device, size_t max_frames, size_t height, size_t width);
void ebcc_hip_destroy(ebcc_hip_ctx *ctx);
/* the context's hipStream_t (so callers can order their own work against it) */
void *ebcc_hip_stream(ebcc_hip_ctx *ctx);
size_t ebcc_hip_workspace_bytes(const ebcc_hip_ctx *ctx);

/* raw device-memory helpers so that C / ctypes callers need no other HIP binding */
void *ebcc_hip_malloc(size_t bytes);
void ebcc_hip_free(void *d_ptr);
int ebcc_hip_memcpy_h2d(void *d_dst, const void *src, size_t bytes);
int ebcc_hip_memcpy_d2h(void *dst, const void *d_src, size_t bytes);

/* ---- residual layer --------------------------------------------------------------------------
 * Batch forms of spiht_encode / spiht_decode, /root/reference/src/spiht/spiht_re.h:20-21
 * (num_stages is fixed to WAVELET_LEVELS = 3, src/ebcc_codec.c:28,748). */

/* d_images: [n_frames][height][width] fp32 in [0,1].  trunc_bits[f] as in spiht_encode.
 * out_streams[f] receives a malloc()'d byte stream of out_sizes[f] bytes (free with free_buffer). */
int ebcc_hip_spiht_encode(ebcc_hip_ctx *ctx, const float *d_images, size_t n_frames, const size_t *trunc_bits,
                          uint8_t **out_streams, size_t *out_sizes);

/* streams[f]/sizes[f]/num_bits[f] as in spiht_decode(buffer_in, input_size, ..., num_bits);
 * d_images_out: [n_frames][height][width] fp32. */
int ebcc_hip_spiht_decode(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes,
                          const size_t *num_bits, size_t n_frames, float *d_images_out);

/* After ebcc_hip_spiht_encode on this context: the image spiht_decode(buf, trunc_bits/8, ..., trunc_bits)
 * would return for a prefix of each stream, rebuilt from the encoder's bookkeeping without parsing
 * (the device form of one probe of the truncation search, src/ebcc_codec.c:778-779). */
int ebcc_hip_spiht_decode_prefix(ebcc_hip_ctx *ctx, size_t n_frames, const size_t *trunc_bits, float *d_images_out);

/* Parity diagnostics: integer wavelet coefficients of the padded grid after load_image + sub_dc +
 * dwt2full + normalize (src/spiht/spiht_re.c:435,461,466,467).  coeffs: host [n_frames][padded pixels],
 * dc: host [n_frames]. */
int ebcc_hip_spiht_coeffs(ebcc_hip_ctx *ctx, const float *d_images, size_t n_frames, int32_t *coeffs, int *dc);
size_t ebcc_hip_padded_pixels(const ebcc_hip_ctx *ctx);

/* Test entry points of the truncation search's probes (src/ebcc_codec.c:745-754, :777-795): they call the launchers the
 * encoder calls, in its order, so that what the tests run is what the search runs (tests/test_probe_residual_gpu.py).
 * _prepare: the residual layer of the encoder for r = d_data - d_decoded (both [n_frames][height][width], 4-byte aligned) with a
 * SPIHT budget of budget_bits[f] bits (> 0; the encoder's is 8 x the base layer's bytes): residual range, padding and DC,
 * analysis, budget, SPIHT.  rmin / rmax / dc (host, [n_frames]) and the streams (malloc'd, free_buffer) come back; the
 * bookkeeping stays in the context for the probes. */
int ebcc_hip_residual_prepare(ebcc_hip_ctx *ctx, const float *d_data, const float *d_decoded, size_t n_frames, const size_t *budget_bits,
                              float *rmin, float *rmax, int *dc, uint8_t **out_streams, size_t *out_sizes);
/* _probe, after _prepare on this context with the same d_data / d_decoded: n_probes probes, probe i = the cut of cut_bits[i] bits
 * (> 128) of frame frame_of[i], counted where active[i] is set, with FrameState::exit_above = exit_above[i] (0: exact).
 * slots == 0: one probe per frame through the one-cut-per-round launcher (n_probes == n_frames, frame_of[i] == i, active the
 * mask); slots != 0: any number of probes a frame, at most 8191 a call, through the cut slots of the look-ahead, set up as the
 * search's advance sets them up.  maxerr_bits[i] = float bits of max |x - (d + r)|, err_sum[i] = sum(x - (d + r)); both arrays are read first and what
 * they hold is what an inactive probe's entry holds afterwards.  0 = ok, 1 = error (a cut of 128 bits or fewer, a frame out of
 * range, a grid the cut slots do not take). */
int ebcc_hip_residual_probe(ebcc_hip_ctx *ctx, const float *d_data, const float *d_decoded, size_t n_frames, int slots, size_t n_probes,
                            const int *frame_of, const size_t *cut_bits, const int *active, const float *exit_above,
                            uint32_t *maxerr_bits, double *err_sum);

/* ---- JPEG 2000 base layer (unit level) ----------------------------------------------------------
 * Batch forms of j2k_encode_internal / j2k_decode_internal, /root/reference/src/ebcc_codec.c:105-180,
 * :1092-1136 (the reference reaches OpenJPEG there).  Frames are scaled to u16 with their own min/max as
 * ebcc_encode does (:675-689) and coded at rate cr[f]; minmax (host, [n][2], may be NULL) returns them. */
int ebcc_hip_j2k_encode(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const float *cr, uint8_t **out_streams,
                        size_t *out_sizes, float *minmax);
/* After ebcc_hip_j2k_encode: the field j2k_decode_internal would return for those codestreams, decoded in
 * place from the encoder's code-block slots; nbad[f] = count(|x - d| > target[f]), err_sum[f] = sum(x - d). */
int ebcc_hip_j2k_emulated_decode(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const float *target,
                                 float *d_out, unsigned long long *nbad, double *err_sum);
/* Test entry point of the rate search's probes (src/ebcc_codec.c:545-596), after ebcc_hip_j2k_encode on this context with the
 * same d_frames, any number of times: one round's work - rate allocation, then the probe decode - through the launchers the
 * search's rounds call (tests/test_probe_j2k_gpu.py).  Frames with active[f] set are probed at rate cr[f] against target[f]
 * with J2kFrame::bad_limit = bad_limit[f] (0: count everything) and J2kFrame::keep = keep[f]; keep_field 0: statistics only,
 * 1: every probed frame stores its field, 2: the frames with keep[f] do.  nbad / err_sum / stream_bytes (host, [n_frames]; the
 * length is the search's own formula) are written for the probed frames only.  d_field_out (device, may be NULL) receives the
 * engine's decoded fields [n_frames][height][width] as they lie after the probe. */
int ebcc_hip_j2k_probe(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const float *cr, const float *target,
                       const uint32_t *bad_limit, const int *keep, const int *active, int keep_field, unsigned long long *nbad,
                       double *err_sum, int *stream_bytes, float *d_field_out);
/* Parity diagnostics of the rate-independent half of the encoder - forward 9/7, quantisation with six fractional bits,
 * tier-1 with its per-pass byte counts, the distortion tables - in plain host arrays (tests/test_j2k_tables_gpu.py compares
 * them with the oracle's analysis stage by stage).  Not on any product path.
 * d_frames given: runs what ebcc_hip_j2k_encode runs before its rate allocation, through the same launchers in the same
 * order (input statistics, analysis, the tier-1 retry; *retried, may be NULL, tells whether that retry ran).  d_frames NULL:
 * launches nothing and returns what stands in the context for its first n_frames frames, e.g. after encodes and probes;
 * coeffs must be NULL then (later decodes reuse the tile buffer).
 * coeffs (may be NULL) / q6 (may be NULL): [n_frames][height][width], the tile buffer with the forward coefficients and the
 * quantised coefficients.  blocks: [n_frames][blocks_per_frame] in packet order (resolution, band, raster);
 * blocks_per_frame must be the frame's number of code-blocks (what ebcc_hip_window_plan returns).  A code-block's cumulative
 * pass rates and distortions are rates / disto [pass_at, pass_at + totalpasses) and its bytes are bytes [byte_at, byte_at +
 * len), packed one behind the other in the order of `blocks`; passes_cap / bytes_cap: room in those arrays (a call that
 * needs more fails).  const_field: [n_frames]; a constant frame is not coded: its code-blocks come back with the
 * geometry, zero passes and zero bytes, its coeffs and q6 zeroed.  0 = ok, 1 = error (bad batch, arrays too small).
 * On a context of ebcc_hip_create_tiles (chunks of `tiles` frames, below): n_frames is a multiple of tiles, frame f is tile
 * f % tiles of chunk f / tiles.  The frames of a chunk are scaled with the chunk's (min, max) and carry the chunk's constant
 * flag, as ebcc_encode scales them, and a frame's rectangles, bands and resolutions are those of its tile position (first
 * row (f % tiles) * height of the image: its own sub-band extents, parities and code-block partition).  blocks_per_frame is
 * ebcc_hip_j2k_blocks_per_frame, the most code-blocks of any tile position; the slots past a tile position's own code-blocks
 * come back with w = h = 0 and the passes and bytes the device holds for them, which must be none. */
typedef struct {
    int x, y, w, h;              /* rectangle in the tile buffer */
    int orient, res;             /* 0 LL, 1 HL, 2 LH, 3 HH; resolution 0 (coarsest) .. 5 */
    int numbps, totalpasses, len;
    int reserved;
    size_t pass_at, byte_at;
} ebcc_hip_j2k_block;
int ebcc_hip_j2k_tables(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, float *coeffs, int32_t *q6,
                        ebcc_hip_j2k_block *blocks, size_t blocks_per_frame, int *rates, double *disto, size_t passes_cap,
                        uint8_t *bytes, size_t bytes_cap, int *const_field, int *retried);
/* the code-block slots of a frame in the context's per-code-block arrays: a frame's number of code-blocks (what
 * ebcc_hip_window_plan returns), on a context of ebcc_hip_create_tiles the most of any tile position; -1: no context */
int ebcc_hip_j2k_blocks_per_frame(const ebcc_hip_ctx *ctx);
/* Parity diagnostics: the context ebcc_encode / ebcc_decode make for chunks of `tiles` frames - one JPEG 2000 image a chunk,
 * one tile a frame, a geometry per tile position (frame f uses number f % tiles) - so that ebcc_hip_j2k_tables can be asked
 * about a tile away from the image's origin (tests/test_tile_positions_gpu.py).  Not on any product path: ebcc_hip_j2k_tables is
 * the only entry point that is defined on such a context (the frame, shard and window entry points refuse it).  tiles == 1 is
 * ebcc_hip_create.  NULL: what
 * ebcc_hip_create refuses, tiles * height above 2047, or tiles > 1 with fewer than 32 rows a tile (no six resolutions in a
 * tile: ebcc_encode refuses such chunks too). */
ebcc_hip_ctx *ebcc_hip_create_tiles(int device, size_t max_frames, size_t height, size_t width, size_t tiles);
/* j2k_decode_internal for a batch of codestreams with (minval, maxval) pairs in minmax [n][2] */
int ebcc_hip_j2k_decode(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                        const float *minmax, float *d_out);

/* Host-only check of the codestream parser behind the decode path (no device needed): 0 = `cs` is accepted as a one-tile
 * codestream of height x width and every code-block entry lies inside it, 1 = rejected, 2 = accepted with an entry out of
 * bounds (never expected).  The reference leaves this to OpenJPEG (/root/reference/src/ebcc_codec.c:1096-1135). */
int ebcc_hip_j2k_parse_check(const uint8_t *cs, size_t n, size_t height, size_t width);

/* ---- frame codec -----------------------------------------------------------------------------
 * Batch forms of ebcc_encode / ebcc_decode (src/ebcc_codec.h:41-42) for frames resident in HBM.
 * config->dims must be {1, height, width} of the context (one frame per stream, as HDF5 chunks of
 * one frame / ebcc_encode_chunking with chunk_dims {1,H,W} produce).  Streams are malloc'd (free_buffer).
 * Return 0 = ok, 1 = error, 2 = NaN/Inf in the input; on failure every stream made so far has been freed
 * (out_streams all NULL).  A batch is coded as EBCC_HIP_SLICES concurrent slices (default: ebcc_hip_default_encode_slices() = 3 from 96 frames on, one slice below),
 * each on its own engine, stream and host thread; results do not depend on the slicing.  The slice engines are created on first use; ebcc_hip_prepare creates them ahead of time for batches of
 * n_frames (part of setting a context up, like ebcc_hip_create).  Returns 0. */
int ebcc_hip_prepare(ebcc_hip_ctx *ctx, size_t n_frames);
/* ebcc_encode / ebcc_decode / the chunking entry points and the HDF5 filter (/root/reference/src/ebcc_codec.h:41-49) keep
 * their engines between calls, one per device and frame geometry - tens of GB of device memory for batches of 256 frames of
 * 721 x 1440.  This gives that memory back; the next call makes the engines again.  Contexts of ebcc_hip_create are not
 * touched. */
void ebcc_hip_release_engines(void);
/* The same for a caller's context: its second engine set (ebcc_hip_encode_shard / ebcc_hip_decode_shard / the host-frames
 * entry points make it on their first call of more than one batch; it is as large as the context) is destroyed, the next
 * such call makes it again (also after a call that found no memory for it). */
void ebcc_hip_release_second_set(ebcc_hip_ctx *ctx);
/* Pageable host memory <-> device memory through the engine's pinned bounce buffers with several copying host threads
 * (what the chunking entry points use for their own arrays): ~3x hipMemcpy on a fresh pageable array.  0 = ok. */
int ebcc_hip_upload(ebcc_hip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int ebcc_hip_download(ebcc_hip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* Frames in pageable host memory <-> streams, any number of frames: what ebcc_encode_chunking / ebcc_decode_chunking
 * (/root/reference/src/ebcc_codec.c:1007-1046, :1322-1449) do between the array and the EBCK container, for callers that
 * keep the chunks themselves (HDF5 direct chunk writes / reads, ebcc_amd/h5_batch.py): staged uploads / downloads, batches
 * of the context's capacity on the two alternating engine sets, the output's pages mapped while the GPU decodes.
 * 0 = ok; on an encode error every stream made so far has been freed. */
int ebcc_hip_encode_host_frames(ebcc_hip_ctx *ctx, const float *h_frames, size_t n_frames, const codec_config_t *config,
                                uint8_t **out_streams, size_t *out_sizes);
int ebcc_hip_decode_host_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                float *h_frames_out);
/* Maps the pages of a host array that is about to receive a download (a fresh allocation of hundreds of MB is unmapped:
 * the download would fault it in page by page): asks for huge pages and touches every page from several threads, returns
 * when done.  DESTINATION arrays only - a zero is written to every page.  Meant to run on a second thread of the caller
 * beside ebcc_hip_decode_frames, as ebcc_decode_chunking (/root/reference/src/ebcc_codec.c:1322-1449) does for the
 * array it returns.  0 = ok. */
int ebcc_hip_prefault(void *h_dst, size_t bytes);
int ebcc_hip_encode_frames(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const codec_config_t *config,
                           uint8_t **out_streams, size_t *out_sizes);
int ebcc_hip_decode_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                           float *d_frames_out);
/* One GPU's share of a large array (BASELINE configs[3]: 4096 frames per GPU): any number of device-resident frames, coded
 * in batches of the context's capacity - the loop a caller of ebcc_hip_encode_frames would write, which is also what
 * ebcc_encode_chunking (/root/reference/src/ebcc_codec.c:1007-1046) does chunk by chunk - but on two alternating engine
 * sets, so that the host part of batch k (the level-22 zstd of the kept residual prefixes, about a quarter of a batch's
 * time, during which its kernels have nothing to do) runs beside the kernels of batch k + 1.  The second engine set is
 * created on first use and lives as long as the context; without memory for it the batches run one after the other.
 * Streams are identical to those of ebcc_hip_encode_frames.  0 = ok; on error every stream made so far has been freed. */
int ebcc_hip_encode_shard(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const codec_config_t *config,
                          uint8_t **out_streams, size_t *out_sizes);
/* The decode counterpart: any number of streams to consecutive frames on the device, batches on the two engine sets side
 * by side (a batch of long residual streams is one wave per frame and leaves most of the chip idle; for host arrays,
 * ebcc_decode_chunking - /root/reference/src/ebcc_codec.c:1322-1449 - downloads one batch beside the next one's kernels the
 * same way).  Same frames as ebcc_hip_decode_frames batch by batch.  0 = ok. */
int ebcc_hip_decode_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                          float *d_frames_out);

/* ---- window decode ---------------------------------------------------------------------------
 * A box [row0, row0 + rows) x [col0, col0 + cols) of every frame - the regional subset of an archive of global fields -
 * decoded from the code-blocks it depends on alone; the reference has no counterpart (ebcc_decode, src/ebcc_codec.h:42,
 * returns whole frames).  The result is bit for bit the crop of what the entry point without a window gives.  Only the
 * tier-1 decode of the needed 64 x 64 code-blocks, the parts of the inverse wavelet levels above the box and the box's rows
 * of the residual layer's last pass run; the field is written straight into the compact output [n][rows][cols] (any 4-byte
 * aligned address), and the host-array form downloads nothing else.  The residual layer's SPIHT decode is one serial chain
 * per frame and runs whole.  Constant fields fill the box with their value; frames without a residual layer, legacy
 * header-less streams and mixed batches work as in the full decode.  Return 0 = ok, 1 = error (ebcc_hip_last_error): an empty
 * window or one not inside the frame is refused before anything is written, malformed streams are refused as by the full
 * decode.
 * Not covered: chunks of several frames (ebcc_decode_chunking's tiled chunks), ebcc_h5_read_frames, the encode side, and
 * the reference-compatible entry points of ebcc_codec.h. */

/* Which code-blocks of a height x width frame a decode of the window [row0,row0+rows) x [col0,col0+cols) needs: the dependency
 * cone of the five inverse 9/7 levels (an even output sample of a level depends on the interleaved positions within +-3, an
 * odd one on those within +-4; the range splits by parity into the low-pass range - the next level's outputs - and the
 * high-pass range).  Host logic, no device work.
 * bands: 16 x {x0, x1, y0, y1}, the needed rectangle of every sub-band in its own coordinates (order of J2kGeom::bands;
 *        x0 == x1: nothing needed).  blocks (may be NULL): per code-block, in decode-table order,
 *        {band, x0, x1, y0, y1, keep}.  Returns the number of code-blocks of the frame, -1 for a window that is empty
 *        or not inside the frame, or a geometry ebcc_hip_create refuses. */
int ebcc_hip_window_plan(size_t height, size_t width, size_t row0, size_t col0, size_t rows, size_t cols,
                         int *bands, int *blocks, size_t max_blocks);
/* ebcc_hip_decode_frames for a window: at most the context's capacity of frames, d_out [n_frames][rows][cols] on the device */
int ebcc_hip_decode_frames_window(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                  size_t row0, size_t col0, size_t rows, size_t cols, float *d_out);
/* ebcc_hip_decode_shard for a window: any number of frames, batches on the two engine sets */
int ebcc_hip_decode_shard_window(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                 size_t row0, size_t col0, size_t rows, size_t cols, float *d_out);
/* ebcc_hip_decode_host_frames for a window: pageable host output [n_frames][rows][cols]; only the window crosses PCIe */
int ebcc_hip_decode_host_frames_window(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                       size_t row0, size_t col0, size_t rows, size_t cols, float *h_out);

/* ---- box-list decode -------------------------------------------------------------------------
 * Any boxes of any frames in one call: a list of boxes of one size rows x cols, each naming the frame it is cut from - the
 * series of K stations through every time step (K boxes per frame), a box that follows a cyclone (one box per frame at a
 * moving origin), random crops of training samples.  Box e is, bit for bit, the crop [row0, row0 + rows) x [col0, col0 + cols)
 * of what ebcc_hip_decode_frames gives for frame `frame`; the output is [n_boxes][rows][cols], box e at index e, at any 4-byte
 * aligned address, and nothing outside it is written, also by a call that fails.
 * A frame is decoded once, from the union of the code-blocks its boxes need, and its residual layer's SPIHT chain runs once
 * whatever the number of its boxes.  A frame that no box names is not read at all: its streams[f] may be NULL with size 0,
 * and nothing of it is parsed, uploaded, decompressed or decoded (it takes no slot of a batch either: the batches of the
 * shard and host forms are cut over the named frames).  Streams of named frames are checked and refused exactly as the
 * full decode does.  Constant fields, frames without a residual layer, legacy streams and mixed batches as in the window decode.
 * `boxes` must be in non-decreasing order of `frame`; repeats, overlaps and identical boxes are allowed, and n_boxes is not
 * limited by the context's capacity (more boxes than it holds frames run as rounds of the inverse wavelet levels over one
 * tier-1 and one SPIHT decode).  Refused with return value 1, a message (ebcc_hip_last_error) and nothing written: n_boxes,
 * rows or cols zero, a box not inside the frame, frame >= n_frames, frames out of order.  One-frame chunks only. */
typedef struct { size_t frame, row0, col0; } ebcc_hip_box;
/* at most the context's capacity of frames (n_frames), d_out on the device */
int ebcc_hip_decode_frames_boxes(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                 const ebcc_hip_box *boxes, size_t n_boxes, size_t rows, size_t cols, float *d_out);
/* any number of frames, batches on the two engine sets; every batch owns a contiguous part of the output */
int ebcc_hip_decode_shard_boxes(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                const ebcc_hip_box *boxes, size_t n_boxes, size_t rows, size_t cols, float *d_out);
/* pageable host output; only the boxes cross PCIe, batch by batch */
int ebcc_hip_decode_host_frames_boxes(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                      const ebcc_hip_box *boxes, size_t n_boxes, size_t rows, size_t cols, float *h_out);
/* Which code-blocks a box-list decode of n_frames frames of height x width reads (host logic, no device work): row f of
 * keep [n_frames][code-blocks] (may be NULL: the call then only counts and checks) is the OR of the keep flags
 * ebcc_hip_window_plan gives for the boxes of frame f, all zero for a frame no box names.  max_blocks: code-blocks a row of
 * keep has room for - fewer than the frame has is refused.  Returns the number of code-blocks of a frame, -1 for anything
 * the decode calls refuse (then keep is not written). */
int ebcc_hip_boxes_plan(size_t height, size_t width, size_t n_frames, const ebcc_hip_box *boxes, size_t n_boxes,
                        size_t rows, size_t cols, uint8_t *keep, size_t max_blocks);

/* ---- placed boxes and slabs of a chunk container -----------------------------------------------
 * A box list whose boxes carry their own extent and their own place in the output: box e is, bit for bit, the crop
 * [row0, row0 + rows) x [col0, col0 + cols) of what ebcc_hip_decode_frames gives for frame `frame`, and its sample (y, x) goes
 * to out[out_offset + y * out_pitch + x] (offsets and pitches in floats; `out` at any 4-byte aligned address).  Only the
 * placed rectangles are written: the gaps between them and everything else of `out` keep their bytes, also when the call
 * fails, and also in the host form.  Target rectangles that overlap are the caller's business: which box wins there is unspecified
 * (with a residual layer, both boxes add to the sample that won).
 * Everything else is the box list's: `boxes` in non-decreasing order of `frame`, repeats allowed, a frame no box names is not
 * read (its streams[f] may be NULL), n_boxes is not limited by the context's capacity (rounds), constant fields fill their
 * rectangle, frames without a residual layer, legacy streams and mixed batches work, streams of named frames are refused
 * exactly as by the full decode.  The batches of the shard and host forms own parts of the list, not of the output; the host
 * form moves the boxes' samples alone over PCIe (compact on the device, placed row by row on the host).
 * Refused with return value 1, a message (ebcc_hip_last_error) and nothing written: n_boxes zero, a box with rows or cols zero
 * or not inside the frame, out_pitch < cols, a box whose last sample lies at or beyond out_floats (the floats `out` holds),
 * frame >= n_frames, frames out of order.  One-frame chunks only.
 *
 * This is what a sub-array ("slab") of an EBCK container (ebcc_encode_chunking / ebcc_encode_chunking_compat,
 * /root/reference/src/ebcc_codec.c:920-1090: every frame cut into spatial chunks, 1024 x 1024 by default, edge chunks padded
 * by index clamping) needs: a chunk is a one-frame stream of the chunk geometry, the slab meets a chunk in one window, and
 * that window lands in its own rectangle of the slab, at the slab's row pitch.  The reference's only read of such a container
 * is ebcc_decode_chunking (src/ebcc_codec.c:1322-1449), every chunk of every time step. */
typedef struct { size_t frame, row0, col0, rows, cols, out_offset, out_pitch; } ebcc_hip_placed_box;
/* at most the context's capacity of frames (n_frames), d_out on the device */
int ebcc_hip_decode_frames_placed(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                  const ebcc_hip_placed_box *boxes, size_t n_boxes, float *d_out, size_t out_floats);
/* any number of frames, batches on the two engine sets */
int ebcc_hip_decode_shard_placed(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                 const ebcc_hip_placed_box *boxes, size_t n_boxes, float *d_out, size_t out_floats);
/* pageable host output */
int ebcc_hip_decode_host_frames_placed(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                       const ebcc_hip_placed_box *boxes, size_t n_boxes, float *h_out, size_t out_floats);

/* The slab [t0, t0 + nt) x [row0, row0 + rows) x [col0, col0 + cols) of an array of `dims` stored in chunks of `chunk_dims`. */
typedef struct { size_t t0, row0, col0, nt, rows, cols; } ebcc_hip_slab;
/* The placed boxes of a slab (host logic, no device work): one box per chunk the slab meets, in increasing linear chunk index
 * (C order over (t, chunk row, chunk column), as the container stores the chunks); `frame` is that index, the window is the
 * slab cut with the chunk's real (unpadded) part, in chunk coordinates, and the placement is that of a compact
 * [nt][rows][cols] output (pitch `cols`).  boxes may be NULL: the call then only counts.  Returns the number of boxes; -1 with
 * `boxes` untouched for an empty slab or one not inside dims, zero dims, chunk_dims[0] != 1, chunk dims ebcc_encode_chunking
 * would refuse, or max_boxes too small. */
long ebcc_hip_slab_plan(const size_t dims[3], const size_t chunk_dims[3], const ebcc_hip_slab *slab,
                        ebcc_hip_placed_box *boxes, size_t max_boxes);
/* dims and chunk_dims of an EBCK container, whose header and chain of `u64 nbytes | stream` entries are checked as
 * ebcc_decode_chunking checks them.  0 = ok, 1 = not a container or a damaged one (message). */
int ebcc_hip_container_info(const uint8_t *data, size_t size, size_t dims[3], size_t chunk_dims[3]);
/* The slab of a container of one-frame chunks, out [nt][rows][cols]: ctx is a context of the chunk geometry, of any
 * capacity (the chunks the slab meets run as batches on the two engine sets).  Of a chunk the slab does not meet only the
 * length field is read.  Refused with a message: data that is not an EBCK container (a plain frame stream has the window
 * decode), chunks of several frames, a context of another geometry, and whatever ebcc_hip_slab_plan refuses. */
int ebcc_hip_decode_container_slab(ebcc_hip_ctx *ctx, const uint8_t *data, size_t size, const ebcc_hip_slab *slab, float *d_out);
int ebcc_hip_decode_container_slab_host(ebcc_hip_ctx *ctx, const uint8_t *data, size_t size, const ebcc_hip_slab *slab, float *h_out);
/* The same on the engines ebcc_decode_chunking keeps between calls (one device): *out_buffer receives a malloc'd array
 * (free_buffer) as with ebcc_decode_chunking, whatever it held.  Returns the number of floats, 0 on failure (message logged). */
size_t ebcc_decode_chunking_slab(uint8_t *data, size_t size, const ebcc_hip_slab *slab, float **out_buffer);

/* ---- container encode from the device --------------------------------------------------------
 * The write side of the above: a [nt][H][W] array of any size that lies on the device -> the EBCK container
 * ebcc_encode_chunking / ebcc_encode_chunking_compat (/root/reference/src/ebcc_codec.c:920-1090) give for the same array on
 * the host, byte for byte.  The padded chunks are gathered on the device, a batch at a time, into the engine set's staging
 * buffer (edge chunks by index clamping, :339-351); no padded copy of the whole array is made, and chunks that are whole
 * frames of the array are coded where they lie.  d_array needs 4-byte alignment only and is never written.
 * Refused with return value 1, a message (ebcc_hip_last_error) and nothing written or allocated for the caller: zero dims,
 * chunk dims ebcc_encode_chunking refuses, dims whose product overflows size_t, chunk_dims[0] != 1 (one-frame chunks only), a
 * context whose frames are not the chunks, first + count beyond the chunk count.  One-frame chunks only. */

/* chunk dims and chunk count ebcc_encode_chunking (compat = 0) / ebcc_encode_chunking_compat (compat = 1) would use for
 * config->dims / config->chunk_dims: host logic, no device.  0 = ok, 1 = whatever those refuse (message). */
int ebcc_hip_container_plan(const codec_config_t *config, int compat, size_t chunk_dims[3], size_t *n_chunks);
/* global min / max of n device floats; 0 = ok, 1 = error, 2 = NaN / Inf present (minmax untouched).  Any 4-byte aligned
 * address; ctx: any context of the device (its stream runs the kernel).  Exact: -0 counts as +0, as < and > see it. */
int ebcc_hip_array_range(ebcc_hip_ctx *ctx, const float *d_data, size_t n, float minmax[2]);
/* unit level: the padded chunks [first, first + count) of d_array [dims] as [count][chunk_dims[1]][chunk_dims[2]] at d_out;
 * chunk_dims[0] must be 1; exactly that many floats are written.  Chunks count in C order over (t, chunk row, chunk column);
 * sample (y, x) of the chunk at (t, r0, c0) is d_array[t][min(r0 + y, H - 1)][min(c0 + x, W - 1)].  d_array and d_out at any
 * 4-byte aligned address; ctx: any context of the device. */
int ebcc_hip_gather_chunks(ebcc_hip_ctx *ctx, const float *d_array, const size_t dims[3], const size_t chunk_dims[3],
                           size_t first, size_t count, float *d_out);
/* the streams of chunks [first, first + count) of the container ebcc_encode_chunking would write for d_array under
 * `config` (dims = the array's, chunk_dims = the chunks'; all zero = refused here).  ctx: a context of the chunk
 * geometry, any capacity: batches of its capacity, gathered into the engine set's staging buffer, on the two alternating
 * sets.  Return and ownership as ebcc_hip_encode_shard (0 / 1 / 2 = NaN or Inf; all streams freed on failure). */
int ebcc_hip_encode_array_chunks(ebcc_hip_ctx *ctx, const float *d_array, const codec_config_t *config,
                                 size_t first, size_t count, uint8_t **out_streams, size_t *out_sizes);
/* the whole container, malloc'd (free_buffer): byte for byte ebcc_encode_chunking (compat = 0) or
 * ebcc_encode_chunking_compat (compat = 1: its default chunk dims, and RELATIVE_ERROR restated as
 * MAX_ERROR with error * (global max - global min), the range taken on the device) of the same array on the host.
 * 0 / 1 / 2 as above (2: nothing is coded, and the process goes on - the host forms exit); *out NULL on failure. */
int ebcc_hip_encode_container(ebcc_hip_ctx *ctx, const float *d_array, const codec_config_t *config, int compat,
                              uint8_t **out, size_t *out_size);

/* ---- frame groups: many variables in one call ------------------------------------------------------
 * An archive step is many variables, a few dozen levels each, every variable with its own rate, bound and often its own
 * mode - temperature to 0.02 K, humidity relative to its range, a mask without a residual layer - and the variables are
 * separate arrays.  A group is one such array with its config; the calls below code the frames of all groups as one list,
 * in batches and slices as the uniform entry points do (the cuts fall where they fall, inside a group if need be), every
 * frame with its group's config.  The reference has one config per call (ebcc_encode, src/ebcc_codec.h:41).
 * Streams come out in group order, frame order within a group.  Frame f of a group is, byte for byte,
 * ebcc_hip_encode_frames of that frame alone with the group's config; for a group with range_of_group it is chunk f of
 * ebcc_hip_encode_container(ctx, group.frames, {dims {n, H, W}, chunk_dims {1, H, W}, ...}, compat = 1).  Results do not
 * depend on how groups, batches, slices and engine sets cut the frames.  The environment switches of the encoder stay
 * process-wide.  A batch whose frames are adjacent in memory is read where it lies; otherwise its runs are copied into the
 * engine set's staging buffer (device forms), or uploaded there run by run (host form).
 * Return and ownership as ebcc_hip_encode_shard: 0 = ok, 1 = error, 2 = NaN / Inf (the message names the group; a group
 * with range_of_group is found before anything is coded); on failure every stream is freed and every out_streams entry is
 * NULL (a list ebcc_hip_groups_check refuses: out_streams is not touched - its length is not known).  One-frame chunks only. */
typedef struct {
    const float   *frames;        /* the group's [n_frames][H][W] floats, 4-byte aligned; device pointer in the frames / shard
                                     forms, host pointer in the host form; read only */
    size_t         n_frames;      /* > 0 */
    codec_config_t config;        /* dims {1, H, W} of the context; base_cr, residual_compression_type, error of this group;
                                     chunk_dims ignored */
    int            range_of_group;/* RELATIVE_ERROR only: error is relative to (max - min) over the whole group, restated as
                                     MAX_ERROR with error * range exactly as ebcc_encode_chunking_compat does
                                     (/root/reference/src/ebcc_codec.c:1078-1087); otherwise ignored, as compat ignores it */
} ebcc_hip_frame_group;
/* total frames <= the context's capacity */
int ebcc_hip_encode_frames_groups(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, uint8_t **out_streams,
                                  size_t *out_sizes);
/* any number of frames, batches on the two engine sets */
int ebcc_hip_encode_shard_groups(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, uint8_t **out_streams,
                                 size_t *out_sizes);
/* groups in pageable host memory, any number of frames; group ranges are taken by host threads, nothing extra is uploaded */
int ebcc_hip_encode_host_frames_groups(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups,
                                       uint8_t **out_streams, size_t *out_sizes);
/* unit level: min / max of n_groups device arrays in ONE launch - d_ptrs[g] (a host array of device pointers, each at any
 * 4-byte aligned address) holds n_floats[g] > 0 floats; minmax [n_groups][2], nonfinite [n_groups].  Exact: -0 counts as +0.
 * A group with a NaN or an Inf sets its flag and leaves its minmax pair untouched; the other groups' results are still
 * exact.  0 = ok, 1 = error, 2 = a flag is set.  ctx: any context of the device. */
int ebcc_hip_group_ranges(ebcc_hip_ctx *ctx, const float *const *d_ptrs, const size_t *n_floats, size_t n_groups, float *minmax,
                          int *nonfinite);
/* Host only, no device: the total number of frames of a list the encode calls above accept for frames of height x width, or
 * -1 with a message for what they refuse before touching a device: n_groups 0 or a null list, a group with n_frames 0 or a
 * null (or misaligned) pointer, config.dims other than {1, height, width}, a geometry ebcc_hip_create refuses, a frame total
 * that overflows.  (The encode calls also refuse a context of another geometry, a context for chunks of several frames, and
 * in the frames form a total beyond the capacity.) */
long ebcc_hip_groups_check(size_t height, size_t width, const ebcc_hip_frame_group *groups, size_t n_groups);

/* ---- audit: the achieved error, measured on the device ---------------------------------------------------
 * The encoder's bound is soft.  ebcc_encode checks max |x - x^| <= target on the reconstruction its search looked at and then folds
 * the mean error into the header's min / max (/root/reference/src/ebcc_codec.c:863-868), which shifts every decoded sample; a
 * search that could not reach the target only logs a warning.  These calls say what a reader of the streams gets: the streams
 * are decoded by the full decode into a buffer of the engine set (made on first use, freed with the set; no decoded frame
 * reaches the caller) and compared with the originals, which are never written.  Per frame: */
typedef struct {
    float    max_abs;   /* max fabsf(x - x^), float arithmetic */
    uint32_t at;        /* the smallest pixel index (row * width + column) where it occurs */
    uint64_t n_over;    /* pixels with fabsf(x - x^) > bound[frame]; 0 without bounds */
    double   sum;       /* sum of (x - x^) and of (x - x^)^2, differences and sums in double */
    double   sum_sq;
    float    x_min;     /* range of the original (-0 counts as +0) */
    float    x_max;
} ebcc_hip_frame_error;
/* The report is the same bytes from run to run and whatever the batch size, the slices, the engine sets and the alignment of
 * the arrays: no atomics, a fixed order of every sum (ebcc_amd/csrc/array_stats.hip: k_frame_errors).  `bound`: host, one float per
 * frame, may be NULL.  Return 0 = ok, 1 = error (streams are refused exactly as ebcc_hip_decode_frames refuses them), 2 = NaN /
 * Inf in the originals (the frames without one are still reported).  One-frame chunks only.
 * unit level, the kernel alone: n_frames frames of height x width at d_x (originals) and d_d (decoded), each at any 4-byte
 * aligned device address; ctx: any context of the device */
int ebcc_hip_frame_errors(ebcc_hip_ctx *ctx, const float *d_x, const float *d_d, size_t n_frames, size_t height, size_t width,
                          const float *bound, ebcc_hip_frame_error *report);
/* at most the context's capacity of frames, originals on the device */
int ebcc_hip_audit_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const float *d_originals,
                          const float *bound, ebcc_hip_frame_error *report);
/* any number of frames, batches on the two engine sets */
int ebcc_hip_audit_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const float *d_originals,
                         const float *bound, ebcc_hip_frame_error *report);
/* originals in pageable host memory, uploaded batch by batch through the staged upload */
int ebcc_hip_audit_host_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const float *h_originals,
                               const float *bound, ebcc_hip_frame_error *report);

/* ---- hard error bound ---------------------------------------------------------------------------------
 * Encode calls whose streams hold their bound for every reader: a batch is audited before its streams leave it, and the frames
 * over their bound are coded again with a smaller error.  Per frame of mode MAX_ERROR or RELATIVE_ERROR, all in float:
 *   T   = error (MAX_ERROR; also the restated bound of a group with range_of_group), error * (x_max - x_min) (RELATIVE_ERROR)
 *   e_0 = error; round k codes the frame with e_k (same mode, same base_cr) and audits that stream: a_k = max_abs
 *   a_k <= T: the frame is met.  Else e_{k+1} = (e_k * (T / a_k)) * 0.9f, and the frame stops as not met when k == max_rounds
 *   (0 means 6) or e_{k+1} is 0 or not below e_k; it then keeps the stream of the round with the smallest a_k, the earliest on ties.
 * Only the offenders of a round are coded again, and the loop runs inside a batch's turn on its engine set: the next batch
 * still runs on the other set, and host frames are still in the set's staging buffer.  Every stream is byte for byte what the
 * plain call gives for the error in error_used; with no offenders the streams are those of the plain call.  NONE-mode frames
 * are never coded again: target = +inf, met = 1, rounds = 0 (achieved is still measured).
 * Return 0 = every frame met, 3 = every frame coded and valid but some not met (report says which), 1 / 2 as the plain calls,
 * with every stream freed.  report: one entry per frame in stream order, may be NULL.  One-frame chunks only.
 * Not covered: chunks of several frames, ebcc_hip_encode_container / ebcc_hip_encode_array_chunks, the reference-compatible entry
 * points and the filter callback, an audit of windows or boxes. */
typedef struct {
    float target;       /* T */
    float achieved;     /* max_abs of the stream the frame keeps */
    float error_used;   /* the error that stream was coded with */
    int   rounds;       /* re-encodes run for the frame */
    int   met;          /* achieved <= target */
} ebcc_hip_bound_report;
int ebcc_hip_encode_shard_groups_hard(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, int max_rounds,
                                      uint8_t **out_streams, size_t *out_sizes, ebcc_hip_bound_report *report);
int ebcc_hip_encode_host_frames_groups_hard(ebcc_hip_ctx *ctx, const ebcc_hip_frame_group *groups, size_t n_groups, int max_rounds,
                                            uint8_t **out_streams, size_t *out_sizes, ebcc_hip_bound_report *report);
/* one array, one config (one group) */
int ebcc_hip_encode_shard_hard(ebcc_hip_ctx *ctx, const float *d_frames, size_t n_frames, const codec_config_t *config, int max_rounds,
                               uint8_t **out_streams, size_t *out_sizes, ebcc_hip_bound_report *report);
int ebcc_hip_encode_host_frames_hard(ebcc_hip_ctx *ctx, const float *h_frames, size_t n_frames, const codec_config_t *config, int max_rounds,
                                     uint8_t **out_streams, size_t *out_sizes, ebcc_hip_bound_report *report);

/* ---- reduce decode: statistics over time from the streams, on the device ------------------------------
 * A mean, a minimum, a maximum, a variance or an exceedance count over time - daily means from hourly steps, a monthly
 * climatology, the diurnal cycle, "days above 30 C" - needs no decoded sample.  Streams go in, per-pixel accumulators come out:
 * the frames (or one window of every frame: only the code-blocks it needs are decoded) are decoded batch by batch into a buffer
 * of the engine set and folded into the accumulators of the bin each frame names; no decoded frame reaches the caller.  The
 * reference has no counterpart (ebcc_decode / ebcc_decode_chunking, src/ebcc_codec.h:42,47, return every sample).
 * The order is the contract: for every bin and pixel the frames of that bin are folded in increasing frame index, one after
 * the other (acc = acc + x), so the accumulators are the same bytes whatever the batch size, the slices, the engine sets, the
 * alignment of the arrays and the split of a series over several calls - the bytes of a plain loop over the decoded fields:
 *   sum += (double) x;  sum_sq += (double) x * (double) x (the product is exact, the sum rounds);  min / max in float, -0
 *   counts as +0 and +0 is written;  over += x > threshold, compared in float.
 * No atomics, and frames never meet in a reduction tree (ebcc_amd/csrc/array_stats.hip: k_time_fold).
 * Not covered: chunks of several frames, a slab of an EBCK container whose region crosses chunks, a host-pointer form, the
 * reference-compatible entry points and the filter callback.  (Statistics over an area per frame: the area series below.) */
#define EBCC_HIP_NO_BIN UINT32_MAX
typedef struct {
    size_t    n_bins, rows, cols;        /* the accumulators are [n_bins][rows][cols] */
    double   *d_sum, *d_sum_sq;          /* device, 8-byte aligned; each may be NULL */
    float    *d_min, *d_max;             /* device, 4-byte aligned; each may be NULL */
    uint32_t *d_over; float threshold;   /* device, may be NULL: frames with sample > threshold */
    uint64_t *count;                     /* host [n_bins]: frames folded into each bin */
} ebcc_hip_time_stats;
/* Host only, no device: the number of frames `bin` names (bin: host [n_frames], NULL = every frame in bin 0, EBCC_HIP_NO_BIN =
 * the frame is skipped), or -1 with a message for what the calls below refuse before touching a device: a null stats or a null
 * count, every device array NULL, n_bins, rows or cols zero, a window [row0, row0 + rows) x [col0, col0 + cols) not inside the
 * height x width frame, a d_sum or d_sum_sq that is not 8-byte aligned or another array that is not 4-byte aligned, a bin >=
 * n_bins, no frame named, a geometry ebcc_hip_create refuses. */
long ebcc_hip_time_stats_check(size_t height, size_t width, const ebcc_hip_time_stats *stats, const uint32_t *bin, size_t n_frames,
                               size_t row0, size_t col0);
/* sums and over = 0, min = +inf, max = -inf, count = 0.  ctx: any context of the device.  0 = ok, 1 = error. */
int ebcc_hip_time_stats_init(ebcc_hip_ctx *ctx, const ebcc_hip_time_stats *stats);
/* unit level, the kernel alone: d_items [n_items][rows][cols] at any 4-byte aligned device address are folded in index order
 * into the bins they name; an item with EBCC_HIP_NO_BIN is not read, a bin no item names is not touched.  The items are never
 * written.  ctx: any context of the device.  Adds to what stats holds (count included).  0 = ok, 1 = error, nothing written. */
int ebcc_hip_time_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, const uint32_t *bin, const ebcc_hip_time_stats *stats);
/* Any number of one-frame streams: the frames `bin` names are decoded - the window [row0, row0 + stats->rows) x [col0, col0 +
 * stats->cols) by the window decode, the whole frame by the full decode when the window is the frame - in batches of the
 * context's capacity on the two engine sets, each into its set's audit buffer (the one ebcc_hip_audit_* use: a context runs
 * one call at a time), and folded.  The decodes of two batches run side by side; the folds take turns in batch order.  A frame
 * with EBCC_HIP_NO_BIN is not read at all: its streams[f] may be NULL with size 0, and it takes no slot of a batch.  The call
 * adds to what stats holds: a series folded by several calls in frame order gives the bytes of one call.
 * Return 0 = ok, 1 = error (ebcc_hip_last_error).  Refused before anything is written, accumulators and count included: what
 * ebcc_hip_time_stats_check refuses for the context's frames, a context for chunks of several frames, a named frame without a
 * stream or with one whose frame header does not parse (truncated, sizes that do not add up).  A stream found damaged inside a
 * batch - its codestream or its residual layer - is refused as ebcc_hip_decode_frames refuses it; a batch folds only after all
 * of it has decoded, so streams that all fail (a context of another geometry) leave everything untouched, but after batches
 * that succeeded the accumulators hold an unspecified mixture and must be initialised again (count is only advanced by a call
 * that succeeds).  Nothing outside the accumulators is written in either case. */
int ebcc_hip_reduce_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin,
                          size_t row0, size_t col0, const ebcc_hip_time_stats *stats);

/* ---- area series: statistics over regions at every time step, from the streams, on the device --------
 * The other question an archive is asked: the area-weighted mean, minimum or maximum over a region for every frame - a
 * global-mean series, an index over a box, a zonal-mean diagram (one region per row), the fraction of an area above a
 * threshold.  Streams go in, n_frames x n_regions records of 32 bytes come out; the bounding box of the regions is decoded
 * (only the code-blocks it needs) batch by batch into a buffer of the engine set and folded there.  No decoded frame reaches
 * the caller.  The reference has no counterpart.
 * The order is the contract: a region's record depends on the region, the weights inside it and the decoded samples inside
 * it, and on nothing else - not on the batch size, the slices, the engine sets, the alignment of any array, the other regions
 * of the list, or whether the frame was decoded whole or as a window.  Here a reduction tree is acceptable where the reduce
 * decode forbids one: frames never meet, and the tree of a region is fixed by the region alone.  It is this fold:
 *   fold64(v, g), v[0 .. n) doubles, g a group size: 64 partial sums, each +0.0 at first; partial l adds the elements i with
 *   (i / g) % 64 == l in increasing i (p = p + v[i]); then p[l] = p[l] + p[l ^ o] for o = 32, 16, 8, 4, 2, 1 (both sides of
 *   an exchange add the same two numbers: all 64 end with the same bits); the result is p[0].
 *   Per pixel (r, c) of a region, in frame coordinates: w = (w_row ? w_row[r] : 1.0) * (d_w_pix ? (double) d_w_pix[r][c] : 1.0).
 *   A pixel with w == 0 takes part in nothing (that is how a mask is expressed).  Otherwise, x the decoded sample (float):
 *     t_sum = (double) x * w;  t_sq = ((double) x * (double) x) * w (the square is exact, one rounding);
 *     t_over = use_threshold && x > threshold ? w : 0.0 (compared in float);  min / max in float by fminf / fmaxf.
 *   Per row of the region: fold64 of the row's terms with g = 4, columns counted from the region's first column.
 *   Per region: fold64 of its row results with g = 1, rows counted from the region's first row.
 *   min / max take the same way (the order does not show in them) and leave with + 0.0f: -0 counts as +0.  A region whose
 *   weights are all zero gives sums of +0.0, min = +inf, max = -inf.  Products and sums are never contracted.
 * No atomics (ebcc_amd/csrc/array_stats.hip: k_area_rows, k_area_fold).
 * Not covered: chunks of several frames, regions that are not boxes beyond what a d_w_pix mask expresses, a host-pointer
 * form, EBCK containers, the reference-compatible entry points and the filter callback. */
typedef struct { size_t row0, col0, rows, cols; } ebcc_hip_region;     /* frame coordinates */
typedef struct {
    size_t n_regions; const ebcc_hip_region *regions;                   /* host; regions may overlap and repeat */
    const double *w_row;     /* host [height], NULL = 1: a weight per row of the frame (cos(latitude)) */
    const float  *d_w_pix;   /* device [height][width], 4-byte aligned, NULL = 1: a weight per pixel (a mask, land fraction) */
    int use_threshold; float threshold;                                 /* over: the weight of the pixels with sample > threshold */
} ebcc_hip_area_spec;
typedef struct { double sum, sum_sq, over; float min, max; } ebcc_hip_area_stat;   /* 32 bytes */
/* Host only, no device: n_regions and (bounding, may be NULL) the bounding box of all regions, or -1 with a message for what
 * the calls below refuse before touching a device: a null spec or list, n_regions == 0, a region that is empty or not inside
 * the height x width frame, a w_row entry (all `height` are looked at) that is negative, a NaN or an Inf, a d_w_pix that is
 * not 4-byte aligned, a geometry ebcc_hip_create refuses, an n_regions whose tables overflow.  d_w_pix is never followed. */
long ebcc_hip_area_check(size_t height, size_t width, const ebcc_hip_area_spec *spec, ebcc_hip_region *bounding);
/* unit level, the kernels alone: d_items [n_items][height][width], whole frames at any 4-byte aligned device address, are
 * folded into out (host, [n_items][n_regions]).  The items and the weights are never written.  ctx: any context of the
 * device.  0 = ok, 1 = error with nothing written: what the check refuses, null or misaligned items, n_items == 0, a d_w_pix
 * with a negative value, a NaN or an Inf inside the bounding box of the regions (one device pass before the fold; weights no
 * region holds are not looked at). */
int ebcc_hip_area_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, size_t height, size_t width, const ebcc_hip_area_spec *spec,
                       ebcc_hip_area_stat *out);
/* Any number of one-frame streams: the bounding box of the regions is decoded - by the window decode, by the full decode when
 * it is the frame - in batches of the context's capacity on the two engine sets, each into its set's audit buffer (a context
 * runs one call at a time), and every batch is folded there into its own rows of out (host, [n_frames][n_regions]): batches
 * take no turns.  Return 0 = ok, 1 = error (ebcc_hip_last_error).  Refused before anything is written: what the check
 * refuses for the context's frames, a context for chunks of several frames, a frame without a stream or with one whose frame
 * header does not parse, a d_w_pix with a negative value, a NaN or an Inf inside the bounding box (one device pass before any
 * decode).  A stream found damaged inside a batch is refused as ebcc_hip_decode_frames refuses it: out is then unspecified
 * within its bounds, and nothing outside it is written. */
int ebcc_hip_series_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const ebcc_hip_area_spec *spec,
                          ebcc_hip_area_stat *out);

/* ---- regrid decode: the same fields on another grid, from the streams, on the device --------
 * The fourth question an archive is asked: 0.25 degree fields conservatively coarsened to 1 degree, k x k block means for an
 * overview, a north-south flip, a sub-sampled or bilinearly interpolated target grid, a centred difference along an axis.
 * Streams go in, n_frames x n_out_rows x n_out_cols floats come out; the bounding box of the supports is decoded (only the
 * code-blocks it needs) batch by batch into a buffer of the engine set and resampled there.  No decoded frame reaches the
 * caller.  The reference has no counterpart.
 * A regrid is a separable linear map with a contiguous support per output position along each axis (ebcc_hip_axis_map).
 * The order is the contract.  For output (R, C) of a frame with decoded float samples x, wr[R][i] and wc[C][j] the packed
 * weights of the row and the column map:
 *   a = +0.0
 *   for i = 0 .. rows.count[R), in increasing i:   r = rows.first[R] + i
 *       t = +0.0;  for j = 0 .. cols.count[C), in increasing j:   t = t + (double) x[r][col(C, j)] * wc[C][j]
 *       a = a + wr[R][i] * t
 *   out[R][C] = (float) a        (round to nearest even; products and sums are never contracted)
 *   col(C, j) = cols.first[C] + j, and (cols.first[C] + j) % width when cols.wrap is set.
 * t depends on (r, C) alone: a two-pass separable form and a fused form that recomputes t where row supports overlap give the
 * same bits (ebcc_amd/csrc/regrid.hip: k_regrid is the fused form).  Weights are used as given: the library does not normalise
 * them.  Every tap takes part - there is no special case for a weight of 0: a term of +-0 never changes an accumulator, since
 * one that starts at +0.0 never becomes -0.0 (so a restatement may pad every support to the longest with weights of 0).  A
 * result depends on the map and on the samples inside its support, and on nothing else - not on the batch size, the slices, the
 * engine sets, the alignment of any array, or whether the frame was decoded whole or as a window.  No atomics, no LDS.
 * Not covered: chunks of several frames, EBCK containers, the reference-compatible entry points and the filter callback, maps
 * that are not separable. */
#define EBCC_HIP_REGRID_MAX_TAPS 256
typedef struct {
    size_t          n_out;    /* output positions along the axis, 1 .. 65535 */
    const uint32_t *first;    /* host [n_out]: first source index of output i's support (any order: a flip is a map) */
    const uint32_t *count;    /* host [n_out]: taps of output i, 1 .. EBCC_HIP_REGRID_MAX_TAPS */
    const double   *weight;   /* host, packed: the weights of output 0, then of output 1, ...; finite, any sign */
    int             wrap;     /* columns only: tap j reads source index (first + j) % width (a cell across the date line) */
} ebcc_hip_axis_map;
typedef struct { ebcc_hip_axis_map rows, cols; } ebcc_hip_regrid_spec;
/* Host only, no device: n_out_rows * n_out_cols and (bounding, may be NULL) the box of the frame the map reads - the whole
 * width when a column support wraps -, or -1 with a message and `bounding` untouched for what the calls below refuse before
 * touching a device: a null spec or table, n_out of 0 or above 65535, a count of 0 or above EBCC_HIP_REGRID_MAX_TAPS, a
 * first >= the extent, a support that leaves the axis (without wrap), wrap set on the row map, a NaN or Inf weight, a geometry
 * ebcc_hip_create refuses, an output size that overflows. */
long ebcc_hip_regrid_check(size_t height, size_t width, const ebcc_hip_regrid_spec *spec, ebcc_hip_region *bounding);
/* unit level, the kernel alone: d_items [n_items][height][width] -> d_out [n_items][n_out_rows][n_out_cols], both on the
 * device at any 4-byte alignment.  The items are never written.  ctx: any context of the device.  0 = ok, 1 = error with
 * nothing written: what the check refuses, null or misaligned pointers, n_items == 0. */
int ebcc_hip_regrid_items(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, size_t height, size_t width,
                          const ebcc_hip_regrid_spec *spec, float *d_out);
/* Any number of one-frame streams: the bounding box of the supports is decoded - by the window decode, by the full decode
 * when it is the frame - in batches of the context's capacity on the two engine sets, each into its set's audit buffer (a
 * context runs one call at a time), and every batch is resampled there into its own frames of d_out (device,
 * [n_frames][n_out_rows][n_out_cols], any 4-byte alignment): batches take no turns.  Return 0 = ok, 1 = error
 * (ebcc_hip_last_error).  Refused before anything is written: what the check refuses for the context's frames, null or
 * misaligned pointers, n_frames == 0, a context for chunks of several frames, a frame without a stream or with one whose frame
 * header does not parse.  A stream found damaged inside a batch (and so every stream, in a context of another geometry) is
 * refused as ebcc_hip_decode_frames refuses it: the output is then unspecified within its bounds, and nothing outside it is
 * written. */
int ebcc_hip_regrid_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                          const ebcc_hip_regrid_spec *spec, float *d_out);
/* The same into pageable host memory: only n_out_rows * n_out_cols floats a frame cross PCIe. */
int ebcc_hip_regrid_host_frames(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames,
                                const ebcc_hip_regrid_spec *spec, float *h_out);

/* ---- quantile decode: order statistics over time per pixel, from the streams, on the device --------
 * The fifth question an archive is asked: how the values at a pixel are distributed over time - the median, the 5th, 90th or
 * 95th percentile per calendar month (the thresholds of TX90p / R95p style indices), an ensemble's quartiles, a return level.
 * Sums, extremes and one exceedance count (the reduce decode) cannot give a percentile, and a full decode of a multi-decade
 * series does not fit a device.  Streams go in, for every bin and rank slot one plane [rows][cols] comes out; no decoded frame
 * reaches the caller.  The reference has no counterpart.
 * The rule is integers' work, so no order rule is needed.  For a bin b take the m frames f with bin[f] == b.  A sample x (float)
 * has the order-preserving key of x + 0.0f:
 *   u = bits(x + 0.0f);  key = (u >> 31) ? ~u : u ^ 0x80000000;  every NaN, whatever its sign and payload: key = 0xFFFFFFFF.
 * So -0 counts as +0, and the order is -inf < negative < 0 < positive < +inf < NaN (that of a sort that puts NaN last).  For
 * a pixel and a rank r (0-based, r < m) the result is the float whose key is the r-th smallest of the m keys, written as that
 * float, +0.0f for a zero and 0x7FC00000 for a NaN: a sample that occurs at the pixel, the canonical zero and NaN aside.
 * Nothing is interpolated here (ebcc_amd/h5_batch.py: BatchCodec.quantiles makes quantiles of the order statistics).
 * The selection is a radix select on the key, most significant digit first, digits of 4 bits: eight passes over the series.
 * In pass s, shift = 28 - 4 s: a sample of bin b counts for slot j if key >> (shift + 4) == prefix[b][j][p] (every sample in
 * pass 0) and adds 1 to hist[b][j][(key >> shift) & 15][p]; then, per (bin, slot, pixel), the first digit d whose running total
 * over the 16 counters exceeds rem is taken: rem -= (total before d), prefix = prefix << 4 | d, counters = 0.  After pass 7
 * prefix is the key.  No atomics (ebcc_amd/csrc/quantile.hip: k_rank_count, k_rank_advance).  The workspace - (16 + 2) * 4
 * bytes per (bin, slot, pixel) - is the context's, grown on demand, set anew by every call and freed with the context.
 * Not covered: a series split over several calls, chunks of several frames, a host-pointer output, EBCK containers, weighted
 * quantiles, quantiles over an area, the reference-compatible entry points and the filter callback. */
#define EBCC_HIP_NO_RANK SIZE_MAX
#define EBCC_HIP_MAX_RANKS 16
typedef struct {
    size_t n_bins, rows, cols, n_ranks;   /* n_ranks: 1 .. EBCC_HIP_MAX_RANKS slots per bin */
    const size_t *rank;                   /* host [n_bins][n_ranks]: 0-based order statistic among the bin's frames; EBCC_HIP_NO_RANK: slot unused */
    float    *d_out;                      /* device [n_bins][n_ranks][rows][cols], 4-byte aligned; an unused slot's plane is never written */
    uint64_t *count;                      /* host [n_bins], written by a call that succeeds: frames of each bin */
} ebcc_hip_time_ranks;
/* Host only, no device: the number of frames `bin` names (bin: host [n_frames], NULL = every frame in bin 0, EBCC_HIP_NO_BIN =
 * the frame is skipped), or -1 with a message for what the calls below refuse before touching a device: a null spec, rank,
 * d_out or count, n_bins, rows or cols zero, n_ranks of 0 or above EBCC_HIP_MAX_RANKS, a d_out that is not 4-byte aligned, sizes
 * that overflow, a geometry ebcc_hip_create refuses, a window [row0, row0 + rows) x [col0, col0 + cols) not inside the height x
 * width frame, a bin >= n_bins, no frame named, a bin with 2^32 frames or more, a rank >= the number of frames its bin is given,
 * every slot unused.  A bin without frames is legal if all its slots are unused. */
long ebcc_hip_time_ranks_check(size_t height, size_t width, const ebcc_hip_time_ranks *spec, const uint32_t *bin, size_t n_frames,
                               size_t row0, size_t col0);
/* Host only: the bytes of workspace a call with this spec needs in its context, n_bins * n_ranks * rows * cols * 72; 0 =
 * overflow or a bad spec. */
size_t ebcc_hip_time_ranks_work_bytes(const ebcc_hip_time_ranks *spec);
/* unit level, the kernels alone: all eight passes over d_items [n_items][rows][cols] at any 4-byte aligned device address; an
 * item with EBCC_HIP_NO_BIN is not read.  The items are never written.  ctx: any context of the device.  0 = ok, 1 = error with
 * nothing written: what the check refuses, null or misaligned items, no memory for the workspace. */
int ebcc_hip_rank_items(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, const uint32_t *bin, const ebcc_hip_time_ranks *spec);
/* Any number of one-frame streams.  Every pass decodes the frames `bin` names - the window [row0, row0 + spec->rows) x [col0,
 * col0 + spec->cols) by the window decode, the whole frame by the full decode when the window is the frame - in batches of the
 * context's capacity on the two engine sets, each into its set's audit buffer, and counts
 * them there (the call holds the device's lock over all eight passes: a context runs one call at a time): the decodes of two batches run side by side, the counts take turns in batch order and share the counters of the
 * primary context.  A frame with EBCC_HIP_NO_BIN is not read at all: its streams[f] may be NULL with size 0; a frame of a bin
 * whose slots are all unused is counted and not read either.  d_out and count
 * are written once, after the last pass.  Return 0 = ok, 1 = error (ebcc_hip_last_error) with nothing written: what the check
 * refuses for the context's frames, a context for chunks of several frames, a named frame without a stream or with one whose
 * frame header does not parse, no memory for the workspace, a stream found damaged inside a batch of any pass (refused as
 * ebcc_hip_decode_frames refuses it; so every stream in a context of another geometry). */
int ebcc_hip_quantile_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin,
                            size_t row0, size_t col0, const ebcc_hip_time_ranks *spec);

/* ---- time-map decode: weighted sums over time per pixel, from the streams, on the device --------
 * The sixth question an archive is asked: a linear functional over time with a weight per frame - the least-squares trend
 * per pixel (the weight is the centred time), the regression of a field on an index series, a composite (weights +-1/m), the
 * annual and semi-annual harmonics (cosine and sine weights), a running mean, a Lanczos filter or an interpolation to other
 * time steps (many outputs, each reading a few neighbouring frames).  The reduce decode adds every frame with weight 1, and
 * the regrid decode's axis maps weight rows and columns: this is the same sparse weighted map for the time axis.  Streams go
 * in, one plane [rows][cols] of doubles per output comes out; no decoded frame reaches the caller.  The reference has no
 * counterpart.
 * The order is the contract, as for the reduce decode.  The map is a list of terms per output (CSR: output o owns the terms
 * start[o] .. start[o + 1)), each a frame and a weight, the frames strictly increasing within an output.  For every output o and
 * pixel p the terms of o are taken in the order of the list:
 *   acc[o][p] = acc[o][p] + weight[t] * (double) x_frame[t][p]
 * The product is rounded to double, then the sum is rounded to double; the two are never contracted into an FMA.  Every listed
 * term takes part - a weight of 0 is no special case: a caller who wants a frame left out leaves the term out.  A frame no term
 * names is not read at all: its streams[f] may be NULL with size 0, and it takes no slot of a batch.  An output without terms
 * is legal and is never touched.  An accumulator that a NaN reaches (a NaN sample, or Inf - Inf) is a NaN, which one is not
 * specified; everything else is specified to the bit.  No atomics, and frames never meet in a reduction tree
 * (ebcc_amd/csrc/time_map.hip: k_time_map; consecutive outputs that name the same frames of a batch are folded together, up to
 * four to a loaded sample, which changes no addition and no order).  So the accumulators are the same bytes whatever the batch
 * size, the slices, the engine sets, the alignment of the arrays, whether the frame was decoded whole or as a window, and the
 * split of a series over several calls made in frame order: a call adds to what d_acc and count hold, and the caller rebases
 * `frame` per call.
 * Not covered: chunks of several frames, EBCK containers, a host-pointer output, float32 accumulators, maps whose weights
 * vary per pixel, the reference-compatible entry points and the filter callback. */
typedef struct {
    size_t          n_out, rows, cols;  /* the accumulators are [n_out][rows][cols] */
    const size_t   *start;              /* host [n_out + 1]: output o owns terms start[o] .. start[o + 1); start[0] == 0 */
    const uint32_t *frame;              /* host [n_terms]: index into the call's stream (item) list, strictly increasing within an output */
    const double   *weight;             /* host [n_terms]: finite, any sign */
    double         *d_acc;              /* device, 8-byte aligned */
    uint64_t       *count;              /* host [n_out]: terms folded into each output */
} ebcc_hip_time_map;
/* Host only, no device: the number of distinct frames the map names, or -1 with a message for what the calls below refuse
 * before touching a device: a null map, start, d_acc or count, a null frame or weight when there are terms, n_out, rows or cols
 * zero, start[0] != 0 or a decreasing start, no term at all, a frame >= n_frames, frames not strictly increasing within an
 * output, a NaN or Inf weight, a d_acc that is not 8-byte aligned, a window [row0, row0 + rows) x [col0, col0 + cols) not inside
 * the height x width frame, sizes that overflow (n_out of 2^32 - 1 or more among them), a geometry ebcc_hip_create refuses. */
long ebcc_hip_time_map_check(size_t height, size_t width, const ebcc_hip_time_map *map, size_t n_frames, size_t row0, size_t col0);
/* d_acc = +0.0, count = 0.  ctx: any context of the device.  0 = ok, 1 = error. */
int ebcc_hip_time_map_init(ebcc_hip_ctx *ctx, const ebcc_hip_time_map *map);
/* unit level, the kernel alone: d_items [n_items][rows][cols] at any 4-byte aligned device address, `frame` indexes the items.
 * An item no term names is not read; the items are never written.  ctx: any context of the device.  Adds to what the map holds
 * (count included).  0 = ok, 1 = error with nothing written: what the check refuses, null or misaligned items. */
int ebcc_hip_time_map_items(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, const ebcc_hip_time_map *map);
/* Any number of one-frame streams: the frames the map names are decoded - the window [row0, row0 + map->rows) x [col0, col0 +
 * map->cols) by the window decode, the whole frame by the full decode when the window is the frame - in batches of the
 * context's capacity on the two engine sets, each into its set's audit buffer (the one ebcc_hip_audit_* use: a context runs
 * one call at a time), and folded.  The decodes of two batches run side by side; the folds take turns in batch order.  The call
 * adds to what the map holds: a series folded by several calls in frame order gives the bytes of one call.
 * Return 0 = ok, 1 = error (ebcc_hip_last_error).  Refused before anything is written, accumulators and count included: what
 * ebcc_hip_time_map_check refuses for the context's frames, a context for chunks of several frames, a named frame without a
 * stream or with one whose frame header does not parse (truncated, sizes that do not add up).  A stream found damaged inside a
 * batch - its codestream or its residual layer - is refused as ebcc_hip_decode_frames refuses it; a batch folds only after all
 * of it has decoded, so streams that all fail (a context of another geometry) leave everything untouched, but after batches
 * that succeeded the accumulators hold an unspecified mixture and must be initialised again (count is only advanced by a call
 * that succeeds).  Nothing outside the accumulators is written in either case. */
int ebcc_hip_project_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, size_t row0, size_t col0,
                           const ebcc_hip_time_map *map);

/* ---- pair decode: co-moments and vector magnitude of two variables over time, from the streams, on the device ----
 * The first question that needs two variables: the correlation of two fields per pixel, a covariance or eddy flux u'v', a
 * lagged auto-covariance (y is x shifted), the mean, maximum and "days above 15 m/s" of the wind speed from u10 / v10.  Two
 * lists of streams go in, per-pixel accumulators come out; no decoded frame reaches the caller.  The reference has no
 * counterpart.
 * The order is the contract, as for the reduce decode.  Two lists of one-frame streams of the same geometry, x and y, have
 * n_steps entries each; step t pairs x[t] with y[t].  For every bin and pixel the steps of that bin are folded in increasing
 * step index, one after the other, with a = (double) x and b = (double) y:
 *   sum_x  = sum_x  + a          sum_y  = sum_y  + b
 *   sum_xx = sum_xx + a * a      sum_yy = sum_yy + b * b      sum_xy = sum_xy + a * b
 *   m      = sqrtf((float)(a * a + b * b))
 *   sum_mag = sum_mag + (double) m;   max_mag = fmaxf(max_mag, m);   over_mag += m > threshold   (compared in float)
 * Every product of two widened floats is exact in double; the sum a * a + b * b rounds once, to double; the result rounds to
 * float (nearest even) and m is the correctly rounded float square root of that float (the library is built with
 * -fhip-fp32-correctly-rounded-divide-sqrt, and the rule relies on that flag and nothing else).  sum_x and sum_xx are
 * therefore the bytes ebcc_hip_reduce_shard gives as sum and sum_sq for x alone.  Not specified: an accumulator a NaN reaches
 * (a NaN sample, Inf - Inf, an Inf magnitude's partner), and the magnitude of a sample pair whose (float)(a * a + b * b) is
 * subnormal; everything else is specified to the bit.  No atomics, and steps never meet in a reduction tree
 * (ebcc_amd/csrc/pair_stats.hip: k_pair_fold).  So the accumulators are the same bytes whatever the batch size, the engine
 * sets, the slices, the alignment of any array, whether the frames were decoded whole or as a window, and the split of a
 * series over several calls made in step order.
 * Not covered: chunks of several frames, EBCK containers, a host-pointer form, x and y of different geometry, the
 * reference-compatible entry points and the filter callback. */
typedef struct {
    size_t    n_bins, rows, cols;                               /* accumulators are [n_bins][rows][cols] */
    double   *d_sum_x, *d_sum_y, *d_sum_xx, *d_sum_yy, *d_sum_xy; /* device, 8-byte aligned; each may be NULL */
    double   *d_sum_mag;                                        /* device, 8-byte aligned; may be NULL */
    float    *d_max_mag;                                        /* device, 4-byte aligned; may be NULL */
    uint32_t *d_over_mag; float threshold;                      /* device, may be NULL: steps with m > threshold */
    uint64_t *count;                                            /* host [n_bins]: steps folded into each bin */
} ebcc_hip_pair_stats;
/* Host only, no device (no device pointer is followed): the number of steps `bin` names (bin: host [n_steps], NULL = every
 * step in bin 0, EBCC_HIP_NO_BIN = the step is skipped), or -1 with a message for what the calls below refuse before touching
 * a device: a null stats or a null count, every device array NULL, n_bins, rows or cols zero, a window [row0, row0 + rows) x
 * [col0, col0 + cols) not inside the height x width frame, a double array that is not 8-byte aligned or another array that is
 * not 4-byte aligned, a NaN threshold when d_over_mag is set, a bin >= n_bins, no step named, a geometry ebcc_hip_create
 * refuses. */
long ebcc_hip_pair_stats_check(size_t height, size_t width, const ebcc_hip_pair_stats *stats, const uint32_t *bin, size_t n_steps,
                               size_t row0, size_t col0);
/* sums and over = 0, max_mag = -inf, count = 0.  ctx: any context of the device.  0 = ok, 1 = error. */
int ebcc_hip_pair_stats_init(ebcc_hip_ctx *ctx, const ebcc_hip_pair_stats *stats);
/* unit level, the kernel alone: d_x_items and d_y_items are [n_items][rows][cols], each at any 4-byte aligned device address;
 * they may be the same array.  Item k of one is paired with item k of the other, in index order, into the bin it names; an item
 * with EBCC_HIP_NO_BIN is not read, a bin no item names is not touched.  The items are never written.  A call that asks for
 * co-moments alone executes no square root, one that asks for the magnitude alone holds no co-moment.  ctx: any context of
 * the device.  Adds to what stats holds (count included).  0 = ok, 1 = error, nothing written. */
int ebcc_hip_pair_fold(ebcc_hip_ctx *ctx, const float *d_x_items, const float *d_y_items, size_t n_items, const uint32_t *bin,
                       const ebcc_hip_pair_stats *stats);
/* Two lists of n_steps one-frame streams: the two frames of every step `bin` names are decoded - the window [row0, row0 +
 * stats->rows) x [col0, col0 + stats->cols) by the window decode, the whole frame by the full decode when the window is the
 * frame - side by side in the same batch (x, y, x, y, ..: a batch holds the context's capacity rounded down to an even number
 * of frames, so an odd capacity works and a capacity of 3 gives one step per batch) on the two engine sets, each into its
 * set's audit buffer, and folded.  The decodes of two batches run side by side; the folds take turns in batch order.  A
 * skipped step is not read at all: both of its stream pointers may be NULL with size 0, and it takes no room in a batch.
 * x_streams == y_streams is legal: sum_xy then carries the bytes of sum_xx.  The call adds to what stats holds: a series folded
 * by several calls in step order gives the bytes of one call.
 * Return 0 = ok, 1 = error (ebcc_hip_last_error).  Refused before anything is written, accumulators and count included: what
 * ebcc_hip_pair_stats_check refuses for the context's frames, null stream or size arrays, a context for chunks of several
 * frames, a context of capacity 1, a named step where either stream is missing or does not parse as a frame stream (the
 * message names the step and says x or y).  A stream found damaged inside a batch behaves as ebcc_hip_reduce_shard documents:
 * the batch is refused as ebcc_hip_decode_frames refuses it, earlier batches may have folded - the accumulators then hold an
 * unspecified mixture and must be initialised again -, and count is only advanced by a call that succeeds. */
int ebcc_hip_pair_shard(ebcc_hip_ctx *ctx, const uint8_t *const *x_streams, const size_t *x_sizes, const uint8_t *const *y_streams,
                        const size_t *y_sizes, size_t n_steps, const uint32_t *bin, size_t row0, size_t col0,
                        const ebcc_hip_pair_stats *stats);

/* ---- spell decode: run lengths and event timing over time per pixel, from the streams, on the device ----
 * When an event happened and how long it lasted: consecutive dry or wet days, the days that lie in warm or cold spells of at
 * least six days, first and last frost, the onset of the growing season, the date of the annual maximum.  Streams go in,
 * per-pixel accumulators come out; no decoded frame reaches the caller.  The reference has no counterpart.
 * The order is the contract, as for the reduce decode.  A step carries a sample x (float), a bin, a label `when` (the caller's:
 * a day of the year, an hour index) and a flag `fresh`.  For every bin and pixel the named steps of that bin are folded one
 * after the other in increasing step index:
 *   event     e = below ? (x < threshold) : (x > threshold), compared in float: a NaN sample is never an event and ends a run
 *   runs      if (fresh) run = 0;  then run = e ? run + 1 : 0
 *             if (run > longest) { longest = run; longest_end = when; }      strictly: among equal runs the earliest stays
 *             if (run == min_len) { spells += 1; spell_steps += min_len; }  else if (run > min_len) spell_steps += 1
 *   events    if (e) { events += 1;  if (first == EBCC_HIP_NO_STEP) first = when;  last = when; }
 *   extremes  if (x > max) { max = x; when_max = when; }   if (x < min) { min = x; when_min = when; }   strictly, in float
 * max and min start at -inf / +inf, the labels at EBCC_HIP_NO_STEP, the counters and run at 0.  -0 compares equal to +0 and +0
 * is written, as the reduce decode does: d_min and d_max are the bytes ebcc_hip_reduce_shard gives over the same frames, and
 * with below == 0 d_events is the bytes of its d_over.  spell_steps counts the steps that lie in runs of at least min_len; a
 * run still open at the end of the series counts as far as it got.  `fresh` is for bins that recur - a month-of-year bin over
 * many years -: the caller marks the first step of each visit to the bin, and the run does not continue from the visit before.
 * The flag of a skipped step is not looked at.
 * The state lives in the accumulators, run included: nothing else is carried from one batch or call to the next.  So the
 * accumulators are the same bytes whatever the batch size, the engine sets, the slices, the alignment of any array, whether
 * the frames were decoded whole or as a window, and the split of a series over several calls made in step order
 * (ebcc_amd/csrc/spell_stats.hip: k_spell_fold; no atomics, and steps never meet in a reduction tree).
 * Not covered: chunks of several frames, EBCK containers, a host-pointer form, events defined on two variables, the
 * reference-compatible entry points and the filter callback. */
#define EBCC_HIP_NO_STEP UINT32_MAX
typedef struct {
    size_t    n_bins, rows, cols;                 /* accumulators [n_bins][rows][cols], device, 4-byte aligned, each may be NULL */
    float     threshold; int below; uint32_t min_len;
    uint32_t *d_run, *d_longest, *d_longest_end, *d_spells, *d_spell_steps;   /* runs */
    uint32_t *d_events, *d_first, *d_last;                                    /* events */
    float    *d_min, *d_max; uint32_t *d_when_min, *d_when_max;               /* extremes */
    uint64_t *count;                              /* host [n_bins]: steps folded into each bin */
} ebcc_hip_spell_stats;
/* Host only, no device (no device pointer is followed): the number of steps `bin` names (bin: host [n_frames], NULL = every
 * step in bin 0, EBCC_HIP_NO_BIN = the step is skipped; when: host [n_frames], NULL = step f has the label f), or -1 with a
 * message for what the calls below refuse before touching a device: what ebcc_hip_time_stats_check refuses - a null stats or a
 * null count, every device array NULL, n_bins, rows or cols zero, a window [row0, row0 + rows) x [col0, col0 + cols) not inside
 * the height x width frame, an array that is not 4-byte aligned, a bin >= n_bins, no step named, a geometry ebcc_hip_create
 * refuses -, and d_longest, d_longest_end, d_spells or d_spell_steps without d_run, d_longest_end without d_longest, d_spells
 * or d_spell_steps with min_len == 0, d_when_max without d_max or d_when_min without d_min, a NaN threshold with any runs or
 * events array, a named step whose label is EBCC_HIP_NO_STEP. */
long ebcc_hip_spell_stats_check(size_t height, size_t width, const ebcc_hip_spell_stats *stats, const uint32_t *bin, const uint32_t *when,
                                size_t n_frames, size_t row0, size_t col0);
/* counters and run = 0, the four labels, first and last = EBCC_HIP_NO_STEP, min = +inf, max = -inf, count = 0.  ctx: any
 * context of the device.  0 = ok, 1 = error. */
int ebcc_hip_spell_stats_init(ebcc_hip_ctx *ctx, const ebcc_hip_spell_stats *stats);
/* unit level, the kernel alone: d_items [n_items][rows][cols] at any 4-byte aligned device address are folded in index order
 * into the bins they name; bin, when (NULL: item k has the label k) and fresh (NULL: no item is fresh) are host arrays of
 * n_items entries.  An item with EBCC_HIP_NO_BIN is not read, a bin no item names is not touched.  The items are never written.
 * A call holds and executes only the families - runs, events, extremes - it has an array of.  ctx: any context of the device.
 * Continues from what stats holds (count included).  0 = ok, 1 = error, nothing written. */
int ebcc_hip_spell_fold(ebcc_hip_ctx *ctx, const float *d_items, size_t n_items, const uint32_t *bin, const uint32_t *when,
                        const uint8_t *fresh, const ebcc_hip_spell_stats *stats);
/* Any number of one-frame streams: the steps `bin` names are decoded - the window [row0, row0 + stats->rows) x [col0, col0 +
 * stats->cols) by the window decode, the whole frame by the full decode when the window is the frame - in batches of the
 * context's capacity on the two engine sets, each into its set's audit buffer, and folded.  The decodes of two batches run
 * side by side; the folds take turns in batch order.  A skipped step is not read at all: its streams[f] may be NULL with size
 * 0, and it takes no slot of a batch.  when == NULL: step f has the label f, its index in `streams`.  The call continues from
 * what stats holds: a series folded by several calls in step order gives the bytes of one call, a run that crosses the cut
 * included.
 * Return 0 = ok, 1 = error (ebcc_hip_last_error).  Refused before anything is written, accumulators and count included: what
 * ebcc_hip_spell_stats_check refuses for the context's frames, null stream or size arrays, a context for chunks of several
 * frames, a named step without a stream or with one whose frame header does not parse (the message names the frame).  A stream
 * found damaged inside a batch behaves as ebcc_hip_reduce_shard documents: the batch is refused as ebcc_hip_decode_frames
 * refuses it, earlier batches may have folded - the accumulators then hold an unspecified mixture and must be initialised
 * again -, and count is only advanced by a call that succeeds. */
int ebcc_hip_spell_shard(ebcc_hip_ctx *ctx, const uint8_t *const *streams, const size_t *sizes, size_t n_frames, const uint32_t *bin,
                         const uint32_t *when, const uint8_t *fresh, size_t row0, size_t col0, const ebcc_hip_spell_stats *stats);

/* Direct-chunk batch path for C callers (netCDF-C / CDO-style pipelines; ebcc_amd/h5_batch.py is the Python form): a dataset
 * whose chunks are single frames - chunk dims (1, ..., 1, H, W), filter 308 as /root/reference/src/h5z_ebcc.c:38-93 reads it -
 * is written / read in device batches instead of one filter callback per chunk (/root/reference/src/h5z_ebcc.c:124-148 is
 * what HDF5 would call per chunk): frames [first_frame, first_frame + n_frames), counted in C order over the leading
 * dimensions, are coded with the dataset's own filter parameters and stored pre-filtered with H5Dwrite_chunk, or fetched with
 * H5Dread_chunk and decoded together.  dset_id: the hid_t (HDF5 >= 1.10) of the open dataset.  HDF5 is not linked: its
 * functions are taken from the libhdf5 the calling process has loaded.  Chunk bytes are identical to the callback's.
 * 0 = ok, 1 = error (logged); NaN / Inf in the frames exits with status 1 like the filter callback. */
int ebcc_h5_write_frames(long long dset_id, size_t first_frame, size_t n_frames, const float *frames);
int ebcc_h5_read_frames(long long dset_id, size_t first_frame, size_t n_frames, float *frames_out);

/* Worker threads of the process-wide host pool that runs the entropy stage (level-22 zstd of the residual prefixes) of
 * every slice of every call: EBCC_HOST_THREADS, else min(affinity mask, TWICE the container's CPU quota (cgroup cpu.max): the
 * stage comes in bursts, a burst may run wider than the quota as long as a period's total stays below it) divided by
 * LOCAL_WORLD_SIZE when the process is one rank of a multi-process job, minus min(slices, 2) for the threads that steer the
 * GPU (none subtracted from a share of 4 or fewer); at most 64. */
int ebcc_hip_host_threads(int slices);
/* Slices an encode batch of 96 frames or more runs as when EBCC_HIP_SLICES is not set (smaller batches: one). */
int ebcc_hip_default_encode_slices(void);
/* Slices an encode batch of n_frames runs as (EBCC_HIP_SLICES and the batch size taken into account). */
int ebcc_hip_encode_slices_for(size_t n_frames);
/* Host-side accounting since the last reset: out[0] usable CPUs (affinity and quota), out[1] CPU quota of the container in
 * CPUs (0: none), out[2] core-seconds spent in zstd, out[3] seconds the slices waited for the zstd workers, out[4] bytes
 * compressed, out[5] entropy batches, out[6] prefix bytes whose compression was proved unnecessary (ebcc_hip_zstd_floor).  bench.py prints them per rank (a run bound by the host's CPUs shows here). */
void ebcc_hip_host_stats(double *out, int reset);
/* Lower bound (bytes) of the zstd frame ZSTD_compress writes for [src, src + n) at any level, from the format alone (the
 * literals no match can cover cost at least their entropy; host_pool.hip: zstd_size_lower_bound); 0 = no bound (n above
 * 4 MB, or a libzstd that may split blocks).  The encoder uses it to decide the reference's "pure base layer beats base +
 * residual" comparison (src/ebcc_codec.c:838) without compressing prefixes that provably lose it. */
size_t ebcc_hip_zstd_floor(const uint8_t *src, size_t n);
/* Host-side check of the arithmetic identities the kernels rely on (the division-free s / 65535.0f of the fused inverse
 * wavelet level, for every s in [0, 65535]); returns the number of violations: 0. */
int ebcc_hip_selfcheck(void);
/* The tier-1 decoder's launch shape for a batch (host logic, no device work): table = the decode table the host parses out of
 * the packet headers, four ints per code-block (offset, segment bytes, bit-planes, passes); out[0..2] = code-blocks (by rank in
 * the longest-first order) that go 1, 2, 4 to a wave, out[3] = lanes per wave of all the others. */
void ebcc_hip_plan_decode_lanes(const int *table, int n_code_blocks, int out[4]);

/* Per-kernel timing with HIP events on the engine's stream (bench.py roofline leg).  Names: "t1_encode",
 * "t1_probe_decode", "t1_decode", "rate_alloc", "j2k_dwt_fwd", "spiht_encode", "frame_errors", "time_fold", "regrid", "rank_count",
 * "rank_advance", "time_map", "pair_fold", "spell_fold".  Process-wide switch. */
void ebcc_hip_timing_enable(ebcc_hip_ctx *ctx, int on);
int ebcc_hip_timing_read(ebcc_hip_ctx *ctx, const char *name, double *total_ms, long *launches);

/* last error text of the calling thread ("" if none) */
const char *ebcc_hip_last_error(void);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* EBCC_HIP_H */
