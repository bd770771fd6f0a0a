/*
 * oracle.h - CPU restatement of the EBCC per-frame codec path.  TEST INFRASTRUCTURE ONLY.
 *
 * Nothing under oracle/ is part of the product: only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load libebcc_oracle.so.  The shipped library
 * (ebcc_amd/libh5z_ebcc.so) never links, includes or dlopens anything from this directory.
 *
 * Parity status
 *   - residual layer (padding, DC removal, CDF 9/7 lifting, truncation to integers, SPIHT
 *     list coder, MSB-first bit I/O, "IMS" header): PINNED bit-exactly against the reference's own
 *     C sources compiled unmodified (oracle/_ref/libspiht_ref.so, recipe in oracle/Makefile) and
 *     against the committed fixtures in tests/golden/ that were generated from that build.
 *   - frame codec orchestration (scaling, residual, both rate searches, truncation search,
 *     header, EBCK container): PINNED against oracle/_ref/libh5z_ebcc_ref.so (reference sources +
 *     the image's OpenJPEG 2.4.0 / zstd 1.4.9) and committed stream fixtures.
 *   - JPEG 2000 base layer: OpenJPEG is an un-vendored submodule of the reference (no pin visible);
 *     parity is defined against OpenJPEG 2.4.0 (/opt/conda/lib/libopenjp2.so.2.4.0 of this
 *     image).  See j2k_oracle.c for what is restated and what is pinned.
 *
 * Every function cites the reference file:line it follows (paths relative to /root/reference).
 */
#ifndef EBCC_ORACLE_H
#define EBCC_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- residual layer (src/spiht/{dwt.h,spiht_re.c,ml.h,bitio.h}) ---- */

/* geometry of the padded transform grid, src/spiht/dwt.h:41-59 */
typedef struct {
    uint32_t size_x, size_y;     /* image width / height                */
    uint32_t extra_x, extra_y;   /* padding to a multiple of 2^(stages+1) */
    uint32_t stride;             /* size_x + extra_x                    */
    uint32_t stages;
} orc_grid_t;

void orc_grid_init(orc_grid_t *g, size_t height, size_t width, size_t stages);

/* load_image + sub_dc + dwt2full + normalize  (src/spiht/spiht_re.c:435,461,466,467).
 * coeffs must hold (size_x+extra_x)*(size_y+extra_y) floats; returns the DC byte. */
int orc_spiht_analysis(const float *image, size_t height, size_t width, size_t stages, float *coeffs);

/* idwt2full + add_dc + crop + /255  (src/spiht/spiht_re.c:508-516); coeffs is destroyed. */
void orc_spiht_synthesis(float *coeffs, size_t height, size_t width, size_t stages, int dc, float *image_out);

/* spiht_encode, src/spiht/spiht_re.c:432-475.  *out is malloc'd. */
void orc_spiht_encode(const float *image, size_t height, size_t width, uint8_t **out, size_t *out_size,
                      size_t trunc_bits, size_t stages);

/* spiht_decode, src/spiht/spiht_re.c:477-520 */
void orc_spiht_decode(const uint8_t *in, size_t in_size, float *image_out, size_t height, size_t width,
                      size_t num_bits);

/* decode only the coefficient grid (no synthesis); returns dc, fills geometry. coeffs malloc'd. */
int orc_spiht_decode_coeffs(const uint8_t *in, size_t in_size, size_t num_bits, orc_grid_t *g, float **coeffs);

/* ---- frame codec (src/ebcc_codec.c) ---- */

#define ORC_NDIMS 3
typedef enum { ORC_NONE = 0, ORC_MAX_ERROR = 1, ORC_RELATIVE_ERROR = 2 } orc_residual_t;

/* same layout as codec_config_t, src/ebcc_codec.h:32-39 */
typedef struct {
    size_t dims[ORC_NDIMS];
    float base_cr;
    int residual_compression_type;
    float residual_cr;
    float error;
    size_t chunk_dims[ORC_NDIMS];
} orc_config_t;

/* J2K back-end used by the frame codec restatement.
 *   0 = j2k_oracle.c restatement (default)
 *   1 = OpenJPEG 2.4.0 loaded with dlopen("libopenjp2.so.7") (the reference's own dependency) */
void orc_set_j2k_backend(int backend);
int  orc_get_j2k_backend(void);

size_t orc_ebcc_encode(const float *data, const orc_config_t *config, uint8_t **out);
size_t orc_ebcc_decode(const uint8_t *data, size_t data_size, float **out);
size_t orc_ebcc_encode_chunking(const float *data, const orc_config_t *config, uint8_t **out);
size_t orc_ebcc_encode_chunking_compat(const float *data, const orc_config_t *config, uint8_t **out);
size_t orc_ebcc_decode_chunking(const uint8_t *data, size_t data_size, float **out);
void   orc_free(void *p);

/* trace of the last orc_ebcc_encode call: probe counts, and which branches of the two error-bound searches
 * (src/ebcc_codec.c:545-596, :730-854) it took.  Mirrored by tests/_lib.py:OrcTrace. */
enum { ORC_EXIT_NONE = 0, ORC_EXIT_BISECT = 1, ORC_EXIT_HI_1000 = 2, ORC_EXIT_LO_FLOOR = 3 };
typedef struct {
    int ran;                       /* the search was called */
    int n_halve, n_double, n_bisect;   /* probes of the loops at :559-563, :565-569, :579-588 */
    int exit;                      /* ORC_EXIT_*: left at :571-574 (cr_hi > 1000, no final probe), or after the
                                      bisection - _LO_FLOOR if the halving loop stopped at cr_lo < 1/2 while infeasible */
    int could_not_reach;           /* the final probe (:590) is below the quantile target (:591-593 warning) */
    float result;                  /* the returned rate */
} orc_search_trace_t;

enum { ORC_RES_NONE = 0, ORC_RES_CONST = 1, ORC_RES_MODE_NONE = 2, ORC_RES_SKIP = 3, ORC_RES_NEED_PURE = 4,
       ORC_RES_TRUNC = 5 };
typedef struct {
    int n_j2k_encodes, n_j2k_decodes, n_spiht_decodes;
    float final_cr;
    size_t coeffs_size, compressed_size, tail_size;
    /* branch record */
    orc_search_trace_t search[2];  /* [0] error-bounded search (:728), [1] pure base layer (:836) */
    int residual;                  /* ORC_RES_*: constant field, NONE mode, base meets the bound (:737), full SPIHT misses
                                      the target (:755-759), truncation bisection ran (:765-796) */
    int trunc_steps;               /* cuts the truncation bisection probed */
    int dropped_small;             /* a prefix of 1..16 bytes was dropped (:811) */
    int fallback_smaller;          /* :838 pure base layer taken because it is smaller */
    int fallback_required;         /* :838 pure base layer taken because the residual layer missed the target */
    int mean_adjusted;             /* :864-868 min / max shifted by the mean error */
} orc_trace_t;
void orc_last_trace(orc_trace_t *t);

/* ---- JPEG 2000 base layer (j2k_oracle.c) ---- */

/* Encode a single-component 16-bit unsigned image exactly the way the reference configures
 * OpenJPEG (src/ebcc_codec.c:105-180): irreversible 9/7, 1 layer, rate = base_cr/2, 6 resolutions,
 * 64x64 code-blocks, LRCP, one tile.  *out malloc'd.  Returns bytes or 0. */
size_t orc_j2k_encode(const uint16_t *img, size_t height, size_t width, float base_cr, uint8_t **out);
/* `tiles` frames of height x width stacked along y, one tile each (ebcc_codec.c:105-180 with n_tiles > 1) */
size_t orc_j2k_encode_tiled(const uint16_t *img, size_t tiles, size_t height, size_t width, float base_cr, uint8_t **out);

/* test hook: called with every code-block's quantised coefficients during orc_j2k_encode / orc_j2k_analysis */
void orc_j2k_set_block_sink(void (*fn)(const int32_t *q, int w, int h, int orient, void *user), void *user);
/* a second hook, called before the first: the code-block's float coefficients as they stand just before quantisation */
void orc_j2k_set_coeff_sink(void (*fn)(const float *cf, int w, int h, int orient, void *user), void *user);
/* Everything of the encoder that does not depend on the rate, per code-block in packet order (resolution, band, raster),
 * for pinning the device analysis: numbps, totalpasses, length, and the per-pass cumulative rates and distortions in rows of
 * 100.  hashes: a polynomial hash of each code-block's bytes.  Returns the number of code-blocks. */
int orc_j2k_analysis(const uint16_t *img, size_t height, size_t width, int *numbps, int *totalpasses, int *lens, int *rates,
                     double *disto, unsigned *hashes);
/* the same with the bytes themselves, one code-block behind the other (b's lens[b] bytes start at the sum of the lengths
 * before it); -1: they need more than `cap` bytes */
int orc_j2k_analysis_bytes(const uint16_t *img, size_t height, size_t width, int *numbps, int *totalpasses, int *lens, int *rates,
                           double *disto, uint8_t *bytes, size_t cap);
/* Both for one tile of an image of `tiles` frames of height x width stacked along y (orc_j2k_encode_tiled): img is the whole
 * stacked image, the tables and both sinks are those of tile `tile` alone, at its place in the image (first row tile * height,
 * so its own sub-band extents, parities and code-block partition).  0: no such tile. */
int orc_j2k_analysis_tiled(const uint16_t *img, size_t tiles, size_t height, size_t width, size_t tile, int *numbps,
                           int *totalpasses, int *lens, int *rates, double *disto, unsigned *hashes);
int orc_j2k_analysis_tiled_bytes(const uint16_t *img, size_t tiles, size_t height, size_t width, size_t tile, int *numbps,
                                 int *totalpasses, int *lens, int *rates, double *disto, uint8_t *bytes, size_t cap);
/* Decode a codestream to int32 samples as OpenJPEG's opj_decode does (src/ebcc_codec.c:1092-1136
 * reads image->comps[0].data).  samples malloc'd. Returns number of pixels or 0. */
size_t orc_j2k_decode(const uint8_t *cs, size_t cs_size, int32_t **samples, size_t *height, size_t *width);

#ifdef __cplusplus
}
#endif
#endif
