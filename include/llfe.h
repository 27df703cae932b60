/*
 * llfe.h -- C ABI of libllfe.so, the MI355X (gfx950) batched image-feature backend.
 *
 * This is the drop-in boundary behind the reference's Python call sites
 * (Kira7dn/Low_Level_Feature_Extraction @ 2025-05-23).  The reference has no FFI of
 * its own -- its "plugin" surface is a set of static Python methods bound by direct
 * import in app/api/v1/endpoints/analyze.py:15-26 -- so each entry point below names
 * the reference function whose native work it replaces.  The Python mirror of those
 * methods lives in low_level_feature_extraction_amd/ and reaches this ABI via ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / numpy types.
 *   - images are BGR, 8-bit, H x W x 3, rows contiguous (stride W*3), batches are
 *     packed N x H x W x 3 (NHWC) with one shared H, W.
 *   - "device" pointers live on the ctx's device (e.g. a torch tensor's data_ptr());
 *     "host" pointers are ordinary CPU memory.
 *   - every call returns LLFE_OK (0) or a negative LLFE_ERR_* code; no exception
 *     crosses the ABI; llfe_last_error(ctx) returns a message for the last failure.
 *   - a ctx is bound to one device and is not thread-safe; use one ctx per host
 *     thread per GPU.  `stream` is a hipStream_t (NULL = the legacy default stream).
 *   - calls are synchronous with respect to their host outputs: when a function
 *     returns, every host output it wrote is valid.
 */
#ifndef LLFE_H
#define LLFE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLFE_ABI_VERSION 3
/* most k-means centres per image (extract_colors(n_colors=...) accepts 1 .. LLFE_MAX_COLORS) */
#define LLFE_MAX_COLORS 32

#define LLFE_OK 0
#define LLFE_ERR_INVALID (-1)
#define LLFE_ERR_HIP (-2)
#define LLFE_ERR_CAPACITY (-3)
#define LLFE_ERR_OOM (-4)
#define LLFE_ERR_UNSUPPORTED (-5)

/* feature mask bits (FeatureType colors / shapes / shadows / fonts) */
#define LLFE_FEATURE_COLORS 1u
#define LLFE_FEATURE_SHAPES 2u
#define LLFE_FEATURE_SHADOWS 4u
/* FontDetector.detect_font's pixel work (font_detector.py:17-67, :109-155): one
 * llfe_font_result per image, fetched with llfe_font_records after the call (the
 * 328-byte llfe_image_result does not change).  The pass runs on the shapes / shadows
 * stream, beside the colour stream's k-means, in either contour mode. */
#define LLFE_FEATURE_FONTS 8u

/* shape type codes (ShapeAnalyzer.analyze_shapes @L159-172 type strings) */
#define LLFE_SHAPE_UNKNOWN 0
#define LLFE_SHAPE_TRIANGLE 1
#define LLFE_SHAPE_RECTANGLE 2
#define LLFE_SHAPE_CIRCLE 3
#define LLFE_SHAPE_POLYGON 4

/* validate_and_preprocess_image modes (app/services/analyze/utils.py:22-28) */
#define LLFE_PRE_NONE 0
#define LLFE_PRE_AUTO 1
#define LLFE_PRE_HIGH_QUALITY 2
#define LLFE_PRE_PERFORMANCE 3

typedef struct llfe_ctx llfe_ctx;
typedef void *llfe_stream; /* hipStream_t */

typedef struct {
    const uint8_t *data;   /* N x H x W x 3 BGR u8 */
    int32_t n, height, width;
    int32_t on_device;     /* 1: device pointer, 0: host pointer */
    /* optional "parity mode" noise: N x H x W x 3 int8 in RGB channel order, i.e.
     * exactly np.random.normal(0, 0.5, (H*W, 3)).astype(np.int8) per image
     * (color_extractor.py:224).  NULL -> on-device counter-based (hashed) noise of the same
     * distribution. */
    const int8_t *noise;
    int32_t noise_on_device;
    int32_t n_colors;      /* extract_colors(n_colors=...) in [1, LLFE_MAX_COLORS]; 0 -> 5 (the default) */
    int64_t index_base;    /* global index of image 0 (seeds are per global index) */
    const int64_t *indices; /* optional (host): global index of each image, overriding
                               index_base + i -- results stay those of each image's own index
                               whatever the batching (a request's image keeps its seeds) */
} llfe_batch;

typedef struct {
    /* colors: _get_dominant_colors + bincount (color_extractor.py:174-236) */
    int32_t n_colors;          /* centres written: K = min(n_colors, U) when K > 1; when K <= 1
                                  (n_colors = 1 or U <= 1) the reference returns every unique
                                  colour with labels [0]*U (color_extractor.py:185-186): here
                                  the first min(U, 5) in np.unique order, counts [U, 0, ...] */
    int32_t counts[LLFE_MAX_COLORS];         /* np.bincount(labels) per centre, k-means order */
    uint8_t centers_rgb[LLFE_MAX_COLORS][3]; /* centers.astype(np.uint8), k-means order */
    uint8_t pad_[4];
    int64_t n_unique;          /* len(np.unique(pixels, axis=0)) */
    double compactness;        /* best cv2.kmeans compactness */
    /* shadows: processed[thresh == 255] sum / size (shadow pyc @L21-24) */
    uint64_t shadow_sum;
    uint64_t shadow_count;
    /* shapes: slice [shape_offset, shape_offset + n_shapes) of the shapes array */
    int64_t shape_offset;
    int32_t n_shapes;
    int32_t n_contours;        /* external contours before the area >= 100 filter */
    /* the reference-shaped summaries, made on the host half of the call in C (no Python):
     * extract_colors' palette rules on the centres / counts above (color_extractor.py:
     * 231-284: most frequent first, '#rrggbb', '#ffffff' / '#000000' dropped, primary, three
     * accents, background by the primary's luminance, is_light_color :67-71) and
     * analyze_shadow_level's level (shadow pyc @L21-31) */
    char primary[8];           /* NUL-terminated; "" when colors were not requested */
    char background[8];        /* "#FFFFFF" or "#000000" (the reference's upper case) */
    char accent[3][8];
    int32_t shadow_level;      /* 0 Low, 1 Moderate, 2 High; -1 when shadows were not requested */
    int32_t pad2_;
} llfe_image_result;

typedef struct {
    int32_t type; /* LLFE_SHAPE_* */
    int32_t x, y, width, height;
    int32_t pad_;
    double border_radius;
    double area;
} llfe_shape;

/* per-kernel timing collected with hipEvents on the launch stream while profiling
 * is enabled (bench.py's roofline numbers) */
typedef struct {
    char name[32];
    int64_t launches;
    double total_ms;
    double bytes;  /* algorithmic HBM bytes attributed to those launches */
} llfe_kernel_stat;

/* one k-means attempt of the last k-means launch (diagnostics, llfe_kmeans_attempts):
 * cv2.kmeans' attempt a (color_extractor.py:192-196) -- its k-means++ centres, the centres
 * and cluster sizes after Lloyd, the Lloyd iterations and the compactness */
typedef struct {
    float pp_centers[5][3];
    float centers[5][3];
    int32_t counts[5];
    int32_t iters;
    double compactness;
} llfe_kmeans_attempt;

/* ---- context ---------------------------------------------------------- */
int llfe_init(int device, llfe_ctx **out);
int llfe_destroy(llfe_ctx *ctx);
const char *llfe_last_error(llfe_ctx *ctx);
int llfe_abi_version(void);
/* file path of the HIP runtime (libamdhip64) the library is bound to.  Device pointers
 * and `stream` handles passed in must come from this same runtime: a process that
 * also uses PyTorch-ROCm loads libllfe after torch, so both share torch's runtime. */
const char *llfe_hip_runtime(void);
/* host threads a new ctx gives its contour pool: the process's share of the usable CPUs
 * -- LLFE_RANK_CPUS when the rank was pinned to its GPU's NUMA node (placement.py), else
 * (affinity mask and cgroup quota) / LOCAL_WORLD_SIZE -- at most 16; LLFE_HOST_THREADS
 * overrides.  Host only. */
int llfe_default_host_threads(void);
/* enable (1) / disable (0) event timing; enabling resets the statistics */
int llfe_set_profiling(llfe_ctx *ctx, int enable);
/* llfe_process_batch runs the colour path on a second stream beside shapes / shadows
 * (1, the default) or everything in order on one stream (0: isolated kernel timings) */
int llfe_set_concurrency(llfe_ctx *ctx, int enable);
/* where llfe_process_batch / llfe_collect_batch run findContours + the shape loop of
 * ShapeAnalyzer.analyze_shapes (shape pyc @L140-181): LLFE_CONTOURS_HOST (default) on the
 * context's host thread pool from the bit-packed mask copied back, overlapping the
 * GPU's k-means; LLFE_CONTOURS_GPU on the GPU (contours_gpu.hip; images up to 4096 wide
 * and 65535 tall, wider ones stay on the host).  Identical results either way.  Initial
 * mode: GPU when the process has fewer than 4 host cores (hardware threads /
 * LOCAL_WORLD_SIZE), else host; LLFE_CONTOURS=host|gpu overrides. */
#define LLFE_CONTOURS_HOST 0
#define LLFE_CONTOURS_GPU 1
/* diagnostic: GPU mode, with every chunk then redone by the host fallback that a chunk
 * the GPU tracer flags as unsupported takes (tests exercise that path with it) */
#define LLFE_CONTOURS_GPU_FORCE_FALLBACK 2
int llfe_set_contour_mode(llfe_ctx *ctx, int mode);
int llfe_get_contour_mode(llfe_ctx *ctx); /* the current mode (or < 0) */
/* batches llfe_submit_batch keeps in flight, each on its own workspace and streams: 2 or
 * 3 (LLFE_INFLIGHT sets a new context's depth, default 2); only with none in flight.  One
 * device pass's workspace is sized within LLFE_WORKSPACE_GB (default 24) per slot, so the
 * device memory held grows with the depth. */
int llfe_set_inflight(llfe_ctx *ctx, int32_t depth);
int llfe_get_inflight(llfe_ctx *ctx); /* the current depth (or < 0) */
/* copies up to cap entries, returns the number of kernels with statistics */
int llfe_kernel_stats(llfe_ctx *ctx, llfe_kernel_stat *out, int32_t cap);
/* host contour pool (LLFE_CONTOURS_HOST), always counted: wall milliseconds the pool spent
 * in contour passes, images traced and the pool's thread count since the last reset
 * (reset != 0 clears after reading).  busy_ms / elapsed wall time near 1 means a
 * workload is bound by the host pool, not the GPU. */
int llfe_host_contour_stats(llfe_ctx *ctx, double *busy_ms, int64_t *images, int32_t *threads, int32_t reset);

/* ---- whole hot path ----------------------------------------------------
 * Replaces, per image of the batch:
 *   ColorExtractor.extract_colors native work  (color_extractor.py:217-236)
 *   ShapeAnalyzer.analyze_shapes               (shape pyc @L125-189)
 *   ShadowAnalyzer.analyze_shadow_level stats  (shadow pyc @L12-24)
 *   FontDetector.detect_font's pixel work      (LLFE_FEATURE_FONTS; records: llfe_font_records)
 * results[n] host; shapes[shape_capacity] host; *shapes_needed = total shapes
 * (LLFE_ERR_CAPACITY when it exceeds shape_capacity; results are still valid). */
int llfe_process_batch(llfe_ctx *ctx, const llfe_batch *batch, uint32_t features, uint64_t seed,
                       llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                       int64_t *shapes_needed, llfe_stream stream);

/* One image of a ragged batch: H x W BGR u8 pixels, rows of W * 3 bytes row_stride bytes
 * apart (0: packed), in host or device memory. */
typedef struct {
    const uint8_t *data;
    int32_t height, width;
    int64_t row_stride;
    int32_t on_device;
    int32_t noise_on_device;
    /* optional parity-mode noise of this image after preprocessing (H' x W' x 3 int8, RGB
     * order, as llfe_batch.noise); give it for every image of the call or for none */
    const int8_t *noise;
} llfe_image_desc;

/* llfe_process_batch for a ragged batch: every image its own size, row
 * stride and memory, plus validate_and_preprocess_image's resize rule applied on the GPU
 * first (preprocessing = LLFE_PRE_NONE / AUTO / HIGH_QUALITY / PERFORMANCE, utils.py:
 * 118-143: INTER_AREA above 2000 px / LANCZOS4 above 4000 / LINEAR above 1000).  Images
 * of one (preprocessed) size share device passes; image i keeps global index
 * index_base + i, so its results equal a one-image call's.  results[i] belongs to
 * images[i]; its shapes are shapes[results[i].shape_offset ...] (LLFE_ERR_CAPACITY and
 * *shapes_needed as llfe_process_batch).  Synchronous. */
int llfe_process_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                        int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                        llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                        int64_t *shapes_needed, llfe_stream stream);

/* llfe_process_images with flags; flags 0 is llfe_process_images itself, an unknown bit is
 * LLFE_ERR_UNSUPPORTED (checked before every other argument).
 * LLFE_IMAGES_COLORS_ONE_PASS: with LLFE_FEATURE_COLORS, the colours of all images of the call
 * come from one device pass whatever their sizes -- one k_uq_scatter, one k_uq_part, one
 * k_uq_gather and one k-means launch -- instead of one pass per size group.  A packed device
 * image is read where it lies (any alignment); a host, strided or resized image is staged
 * packed at a 16-byte aligned offset of one staging buffer.  The per-image arrays of the
 * pass keep the strides of its largest image (llfe_colors_images_layout); a call that does not
 * fit one workspace (LLFE_WORKSPACE_GB, at most 4096 images) is cut into consecutive passes.
 * The other features of the call still run by size group, and every field of every result is
 * bit for bit what flags 0 gives. */
#define LLFE_IMAGES_COLORS_ONE_PASS 1u
int llfe_process_images_flags(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                              int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                              llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                              int64_t *shapes_needed, llfe_stream stream, uint32_t flags);

/* The plan of the colour passes LLFE_IMAGES_COLORS_ONE_PASS runs (host only, no ctx). */
typedef struct {
    int64_t pixels;        /* P = height * width after preprocessing */
    int64_t field_pixels;  /* the image's own noise-field length, P rounded up to 16 */
    int64_t stage_offset;  /* byte offset in its pass's staging buffer (a multiple of 16); -1: read in place */
    int32_t height, width; /* after preprocessing */
    int32_t steps;         /* scatter steps of 4096 pixels */
    int32_t pass;          /* the pass it belongs to */
    int32_t resized;       /* the preprocessing rule resizes it */
    int32_t pad_;
} llfe_color_image;        /* 48 bytes */
typedef struct {
    int32_t image;              /* index in the call */
    int32_t first_step, steps;  /* the scatter steps one workgroup takes (steps >= 1) */
} llfe_color_work;              /* 12 bytes */
typedef struct {
    int32_t first, count;            /* images [first, first + count) of the call */
    int32_t work_first, work_count;  /* its entries of the work table */
    int32_t tab_steps;               /* steps of its largest image: the run-table row */
    int32_t pad_;
    int64_t max_pixels;              /* its largest image */
    int64_t key_stride, cube_stride, cell_stride; /* the common per-image strides, from max_pixels */
    int64_t stage_bytes;             /* its staging buffer */
} llfe_color_pass;                   /* 64 bytes */
/* images / work / passes may each be NULL (counts only: *n_work, *n_passes).  LLFE_ERR_INVALID
 * for what llfe_process_images rejects (a bad descriptor, a bad preprocessing mode);
 * LLFE_ERR_CAPACITY when work_capacity or pass_capacity is short (the counts are still set).
 * Passes are consecutive runs of the input order: a pass grows while its image count stays
 * within llfe_batch_capacity of its largest image. */
int llfe_colors_images_layout(const llfe_image_desc *descs, int32_t n, int32_t preprocessing,
                              llfe_color_image *images, llfe_color_work *work, int64_t work_capacity,
                              int64_t *n_work, llfe_color_pass *passes, int32_t pass_capacity, int32_t *n_passes);

/* llfe_process_images_flags with a second flag word for the shapes / shadows route; an unknown
 * bit in either word is LLFE_ERR_UNSUPPORTED (checked before every other argument).
 * colors_flags: the flags of llfe_process_images_flags.
 * LLFE_IMAGES_SHAPES_ONE_PASS (shapes_flags): with LLFE_FEATURE_SHAPES and / or
 * LLFE_FEATURE_SHADOWS, the shapes and shadows of all images of the call come from one device
 * pass whatever their sizes -- one stencil launch, one hysteresis + dilate sequence, one D2H of
 * the packed masks and the shadow sums, one fan-out over the host contour pool -- instead of one
 * of each per size group.  Images are read in place or staged as for the colour pass (an image
 * both one-pass routes stage is staged twice).  A call that does not fit one workspace
 * (llfe_shapes_images_layout) is cut into consecutive passes.  Fonts still run by size group.
 * While the context traces contours on the GPU (llfe_set_contour_mode), a call that asks for
 * shapes takes the size-grouped route for shapes and shadows.  Every field of every result is
 * bit for bit what shapes_flags 0 gives. */
#define LLFE_IMAGES_SHAPES_ONE_PASS 1u
int llfe_process_images_routes(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                               int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                               llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                               int64_t *shapes_needed, llfe_stream stream, uint32_t colors_flags,
                               uint32_t shapes_flags);

/* The plan of the passes LLFE_IMAGES_SHAPES_ONE_PASS runs (host only, no ctx). */
typedef struct {
    int64_t pixels;         /* height * width after preprocessing */
    int64_t class_offset;   /* of its class map (one byte a pixel) in its pass's, a multiple of 16 */
    int64_t word_offset;    /* of its height * ceil(width / 64) mask words in its pass's */
    int64_t stage_offset;   /* byte offset in its pass's staging buffer (a multiple of 16); -1: read in place */
    int32_t height, width;  /* after preprocessing */
    int32_t strips, segs, seg_rows; /* the stencil's 240-column strips and row segments of seg_rows rows */
    int32_t tiles_x, tiles_y;       /* 64 x 64 hysteresis tiles */
    int32_t first_tile;     /* id of its tile (0, 0) among its pass's tiles */
    int32_t first_part;     /* its first shadow partial = its first work entry within its pass */
    int32_t pass;           /* the pass it belongs to */
    int32_t resized;        /* the preprocessing rule resizes it */
    int32_t pad_;
} llfe_shape_image;         /* 80 bytes */
typedef struct {
    int32_t image;          /* index in the call */
    int32_t strip, seg;     /* one stencil wave: columns [240 strip, +240), rows [seg_rows seg, +seg_rows) */
} llfe_shape_work;          /* 12 bytes */
typedef struct {
    int32_t first, count;            /* images [first, first + count) of the call */
    int32_t work_first, work_count;  /* its entries of the work table */
    int32_t tiles;                   /* its hysteresis tiles (< 524288: the ids tile * 4096 + node are int) */
    int32_t pad_;
    int64_t class_bytes;             /* its class map (every image's rounded up to 16) */
    int64_t words;                   /* its mask words */
    int64_t first_word;              /* the words of the passes before it (llfe_shape_bits_images) */
    int64_t stage_bytes;             /* its staging buffer */
    int64_t workspace_bytes;         /* what the budget counts (below) */
} llfe_shape_pass;                   /* 64 bytes */
/* Same calling convention as llfe_colors_images_layout.  Passes are consecutive runs of the input
 * order.  A pass grows while (a) workspace_bytes = 3 class_bytes (class map, u16 labels) + 29204
 * tiles (per tile: 4096 x 7 bytes of union-find parents, root flags and root lists, 512 of promoted
 * bits, 20 of counts, lists and flags) + 16 words (edge and mask words) + stage_bytes + 8
 * work_count (shadow partials) stays within LLFE_WORKSPACE_GB (default 24) x 10^9 bytes -- the
 * budget of llfe_batch_capacity -- and (b) it has fewer than 524288 tiles (every image has at
 * least as many tiles as stencil waves, so the work table is bounded with them).  An image that
 * alone exceeds (a) is a pass of its own. */
int llfe_shapes_images_layout(const llfe_image_desc *descs, int32_t n, int32_t preprocessing,
                              llfe_shape_image *images, llfe_shape_work *work, int64_t work_capacity,
                              int64_t *n_work, llfe_shape_pass *passes, int32_t pass_capacity, int32_t *n_passes);

/* Asynchronous form (serving loops): llfe_submit_batch enqueues the device work of one
 * batch (n <= one device pass) and returns a ticket; llfe_collect_batch (tickets in
 * submission order) waits for it, traces contours and fills results / shapes exactly as
 * llfe_process_batch would.  At most two batches are in flight; batch k + 1 runs on the
 * second workspace, so its kernels start in the tail of batch k's k-means.  The input
 * (and parity noise) must stay valid until the ticket is collected.  On
 * LLFE_ERR_CAPACITY the ticket stays collectable with a larger shapes buffer. */
int llfe_submit_batch(llfe_ctx *ctx, const llfe_batch *batch, uint32_t features, uint64_t seed, llfe_stream stream,
                      int64_t *ticket);
int llfe_collect_batch(llfe_ctx *ctx, int64_t ticket, llfe_image_result *results, llfe_shape *shapes,
                       int64_t shape_capacity, int64_t *shapes_needed);

/* llfe_submit_batch for n separately allocated images of ONE size (the request path:
 * concurrent /analyze requests -- app/api/v1/endpoints/analyze.py:63-129, one image per
 * request -- sharing one launch, MicroBatcher).  The images (host or device, any row
 * stride, no parity noise) are gathered on the submit's stream into the in-flight
 * slot's own input buffer (device sources: one gather kernel; host sources: 2-D
 * copies), then run exactly as llfe_submit_batch; image i carries global index
 * indices[i] (its noise / k-means seeds), so its results equal a one-image call's.
 * Collect with llfe_collect_batch.  The sources must stay valid until the ticket is
 * collected; the library keeps its own copy of `images` and `indices`. */
int llfe_submit_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features, int32_t n_colors,
                       uint64_t seed, const int64_t *indices, llfe_stream stream, int64_t *ticket);
/* images of h x w one device pass takes: the largest n llfe_submit_batch /
 * llfe_submit_images accept (the workspace budget, LLFE_WORKSPACE_GB); < 0 on bad sizes */
int llfe_batch_capacity(int32_t h, int32_t w);

/* ---- stage entry points (parity tests; device in/out unless noted) ------
 * The ones that use the context's workspace (llfe_shape_mask, llfe_canny,
 * llfe_hysteresis, llfe_shadow_stats, llfe_shape_bits_images, llfe_shadow_stats_images,
 * llfe_hysteresis_images, llfe_color_unique, llfe_kmeans, llfe_find_contours_gpu,
 * llfe_shapes_from_masks_gpu, llfe_font_detect, llfe_font_bits) and llfe_process_images return LLFE_ERR_INVALID while a
 * batch submitted with llfe_submit_batch is not yet collected. */
/* gray = cvtColor(BGR2GRAY); out = GaussianBlur(gray, (5,5), 0)
 * (shape pyc @L18-21, shadow pyc @L8-9) */
int llfe_gray_blur5(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *blurred, int32_t n, int32_t h, int32_t w,
                    llfe_stream stream);
/* dilate(Canny(blur5(gray), 50, 150), ones(3,3)) as 0/255 u8 (shape pyc @L6-30) */
int llfe_shape_mask(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *mask, int32_t n, int32_t h, int32_t w,
                    llfe_stream stream);
/* Canny(blur5(gray), 50, 150) as 0/255 u8: the shape mask before its dilation */
int llfe_canny(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *edges, int32_t n, int32_t h, int32_t w,
               llfe_stream stream);
/* The hysteresis of llfe_canny / llfe_shape_mask on the caller's class maps (the
 * counterpart of llfe_find_contours_gpu, which takes host masks).  classes: HOST n x h x w
 * bytes, each 0 (weak), 1 (none) or 2 (strong); any other byte is LLFE_ERR_INVALID, found
 * by a host scan before any launch.  edges (what llfe_canny gives after its stencil) and
 * mask (edges dilated 3x3, what llfe_shape_mask gives) are HOST n x h x w buffers of
 * 0/255; either may be null, not both.  tile_flags == 0: every 64 x 64 tile is listed;
 * != 0: only the tiles holding a byte != 1, through the flag bytes the stencil would have
 * written.  n above llfe_batch_capacity(h, w) is LLFE_ERR_UNSUPPORTED. */
int llfe_hysteresis(llfe_ctx *ctx, const uint8_t *classes, int32_t n, int32_t h, int32_t w, int32_t tile_flags,
                    uint8_t *edges, uint8_t *mask);
/* dilate(src, ones(3,3)) of n h x w u8 images (any values; out-of-image never wins);
 * src and dst must not alias */
int llfe_dilate3(llfe_ctx *ctx, const uint8_t *src, uint8_t *dst, int32_t n, int32_t h, int32_t w,
                 llfe_stream stream);
/* Canny NMS classes before hysteresis: 0 weak, 1 suppressed, 2 strong */
int llfe_edge_classes(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *classes, int32_t n, int32_t h, int32_t w,
                      llfe_stream stream);
/* FontDetector.preprocess_image (app/services/analyze/font_detector.py:17-37):
 * adaptiveThreshold(cvtColor(BGR2GRAY), 255, GAUSSIAN_C, THRESH_BINARY_INV, 11, 2) as
 * 0/255 u8; bgr and mask are device pointers (n x h x w x 3 / n x h x w). */
int llfe_font_binary(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *mask, int32_t n, int32_t h, int32_t w,
                     llfe_stream stream);
/* FontDetector.detect_font on the device (app/services/analyze/font_detector.py:39-67
 * detect_text_regions, :109-155 detect_font): per image the external contours of the
 * binary in cv2's list order, the text regions among their bounding rectangles
 * (0.1 < w / float(h) < 15 and h > 8), the largest one (max by w * h, the first in list
 * order on ties) and the exact sum of cvtColor(BGR2GRAY) over its rectangle, from which
 * the caller makes np.mean as (double)gray_sum / (width * height).
 * bgr (n x h x w x 3) and binary (n x h x w, nonzero = foreground) are device pointers;
 * binary may be NULL: it is then llfe_font_binary(bgr); with a binary, bgr may be NULL
 * (regions only: every gray_sum is 0).  results (n records) and regions
 * (4 x int32 x, y, w, h per region, the images' lists one after another; may be NULL when
 * only the records are wanted) are host pointers.  *regions_needed (may be NULL) receives
 * the total number of regions; when regions is given and region_capacity is short the
 * call returns LLFE_ERR_CAPACITY with results still valid.  LLFE_ERR_UNSUPPORTED: width
 * above 4096, height above 65535, or a mask the border follower gives up on. */
typedef struct {
    int32_t n_contours;      /* external contours of the binary */
    int32_t n_regions;       /* those passing the aspect / height filter */
    int32_t x, y, width, height; /* largest region (first in cv2 order on equal w*h); zeros when n_regions == 0 */
    int64_t region_offset;   /* this image's regions are regions[4*region_offset ...], n_regions of them, cv2 order */
    uint64_t gray_sum;       /* sum of BGR2GRAY over the largest region's rectangle; 0 when none */
} llfe_font_result;          /* 40 bytes */
int llfe_font_detect(llfe_ctx *ctx, const uint8_t *bgr, const uint8_t *binary, int32_t n, int32_t h, int32_t w,
                     llfe_font_result *results, int32_t *regions, int64_t region_capacity,
                     int64_t *regions_needed, llfe_stream stream);
/* The font binary of llfe_font_binary as bit rows, in one kernel (k_font_bits; the front end
 * of LLFE_FEATURE_FONTS): bits is device n x h x ceil(w / 64) u64, bit x & 63 of word
 * x >> 6 is pixel x (set = 255 in llfe_font_binary's mask), every bit at x >= w is 0.
 * bgr is a device pointer (n x h x w x 3). */
int llfe_font_bits(llfe_ctx *ctx, const uint8_t *bgr, uint64_t *bits, int32_t n, int32_t h, int32_t w,
                   llfe_stream stream);
/* the same for n separately allocated device images of one size: images is a HOST array of
 * n device pointers, each a packed h x w x 3 image (what llfe_submit_images reads in place) */
int llfe_font_bits_images(llfe_ctx *ctx, const uint8_t *const *images, uint64_t *bits, int32_t n, int32_t h,
                          int32_t w, llfe_stream stream);
/* host only: the column-strip width and row-segment height k_font_bits uses for an h x w
 * image (one wave per strip and segment), so that tests can stand on its seams */
int llfe_font_bits_tiling(int32_t h, int32_t w, int32_t *strip_w, int32_t *seg_h);
/* font records of a call that ran with LLFE_FEATURE_FONTS.
 * ticket = a collected llfe_submit_* ticket, or LLFE_LAST_CALL for the last
 * llfe_process_batch / llfe_process_images.  n must equal that call's image count; out
 * receives n records in the call's image order (region_offset is 0: no region lists on this
 * path; for llfe_process_images the rectangle is in the preprocessed image's coordinates).
 * Valid from the call's return (the ticket's collect) until the next process / collect on
 * this context.  LLFE_ERR_INVALID for an uncollected, unknown or expired ticket, a call that
 * ran without the bit, or a wrong n. */
#define LLFE_LAST_CALL (-1)
int llfe_font_records(llfe_ctx *ctx, int64_t ticket, llfe_font_result *out, int32_t n);
/* TextExtractor.preprocess_image (app/services/analyze/text_extractor.py:15-46): gray
 * (cvtColor BGR2GRAY for 3 / 4 channels, the image itself for 1), INTER_CUBIC upscale by
 * max(2, 300 / w, 100 / h) when h < 30 or w < 100, Otsu THRESH_BINARY, bitwise_not when
 * mean(binary) > 127.  img: device h x w x channels u8; out: device out_h x out_w u8
 * (llfe_text_size); *threshold (host, may be NULL) receives Otsu's threshold. */
int llfe_text_binary(llfe_ctx *ctx, const uint8_t *img, int32_t h, int32_t w, int32_t channels, uint8_t *out,
                     int32_t *threshold, llfe_stream stream);
/* output size of llfe_text_binary: returns 1 when the image is upscaled, 0 when not
 * (text_extractor.py:31-37; saturate_cast<int> of w * scale, h * scale), negative for
 * invalid sizes or an upscaled side past INT32_MAX. Host only. */
int llfe_text_size(int32_t h, int32_t w, int32_t *out_h, int32_t *out_w);
/* sums[n], counts[n] host: adaptive-threshold shadow statistics (shadow pyc @L15-21) */
int llfe_shadow_stats(llfe_ctx *ctx, const uint8_t *bgr, uint64_t *sums, uint64_t *counts, int32_t n, int32_t h,
                      int32_t w, llfe_stream stream);
/* llfe_shape_mask for n images that each have their own size, row stride and memory (descriptors
 * as llfe_process_images, no preprocessing), through the passes of LLFE_IMAGES_SHAPES_ONE_PASS.
 * bits: HOST u64 words, bit x & 63 of word x >> 6 of a row is pixel x (set = 255 in
 * llfe_shape_mask's mask); image i's height * ceil(width / 64) words begin at its pass's
 * first_word + its word_offset (llfe_shapes_images_layout).  bits_capacity_words below the
 * layout's total is LLFE_ERR_CAPACITY. */
int llfe_shape_bits_images(llfe_ctx *ctx, const llfe_image_desc *descs, int32_t n, uint64_t *bits,
                           int64_t bits_capacity_words, llfe_stream stream);
/* llfe_shadow_stats for such a list: sums[n], counts[n] host */
int llfe_shadow_stats_images(llfe_ctx *ctx, const llfe_image_desc *descs, int32_t n, uint64_t *sums,
                             uint64_t *counts, llfe_stream stream);
/* llfe_hysteresis for n class maps of any sizes in one ragged pass: class_maps[i] is a HOST
 * heights[i] x widths[i] map of bytes 0 / 1 / 2 (any other byte is LLFE_ERR_INVALID, found before
 * any launch).  bits_edges / bits_mask (either may be null, not both): HOST words as
 * llfe_shape_bits_images lays them out for images of these sizes (the edges, and the edges
 * dilated 3 x 3); bits_capacity_words as there.  tile_flags as llfe_hysteresis.  A list that does
 * not fit one pass is LLFE_ERR_UNSUPPORTED. */
int llfe_hysteresis_images(llfe_ctx *ctx, const uint8_t *const *class_maps, const int32_t *heights,
                           const int32_t *widths, int32_t n, int32_t tile_flags, uint64_t *bits_edges,
                           uint64_t *bits_mask, int64_t bits_capacity_words);
/* noise + np.unique(axis=0) (color_extractor.py:220-225,177).  keys: device
 * n x (h*w) u32 (R<<16|G<<8|B ascending, first n_unique[i] valid); n_unique host. */
int llfe_color_unique(llfe_ctx *ctx, const llfe_batch *batch, uint64_t seed, uint32_t *keys, int64_t *n_unique,
                      llfe_stream stream);
/* llfe_color_unique for n images that each have their own size, row stride and memory
 * (descriptors as llfe_process_images, no preprocessing), through the colour passes of
 * LLFE_IMAGES_COLORS_ONE_PASS.  Image i carries global index index_base + i.  keys: device
 * n x key_stride u32, key_stride >= the largest pixel count; image i's keys start at
 * keys + i * key_stride (first n_unique[i] valid); n_unique host. */
int llfe_color_unique_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint64_t seed,
                             int64_t index_base, uint32_t *keys, int64_t key_stride, int64_t *n_unique,
                             llfe_stream stream);
/* cv2.kmeans(float32(keys->RGB), K=min(n_colors,U), None, (EPS+MAX_ITER,200,0.2), 10,
 * KMEANS_PP_CENTERS) per image (color_extractor.py:189-197).  keys device
 * (n x key_stride), n_points host; results host (colour fields only). */
int llfe_kmeans(llfe_ctx *ctx, const uint32_t *keys, int64_t key_stride, const int64_t *n_points, int32_t n,
                int32_t n_colors, uint64_t seed, int64_t index_base, llfe_image_result *results,
                llfe_stream stream);
/* extract_colors' palette rules alone (color_extractor.py:231-284; host, no context):
 * k centres (RGB u8) and counts in k-means order -> r's primary / background / accent, as
 * llfe_process_batch fills them (the other fields of r are left as they are). */
int llfe_palette_rules(const uint8_t *centers_rgb, const int32_t *counts, int32_t k, llfe_image_result *r);
/* Diagnostics: the 10 attempt records (llfe_kmeans_attempt) of each of the first n images
 * of the last k-means launch on this context (n <= its size): the last chunk of
 * llfe_process_batch / llfe_process_images, an llfe_kmeans call, or the ticket submitted
 * last (LLFE_ERR_INVALID until every ticket is collected), for n_colors <= 5 (k_kmeans, with
 * or without cube tables), into out[n * 10] (host).  Replaces nothing in the
 * reference: cv2.kmeans only returns the best attempt (color_extractor.py:194). */
int llfe_kmeans_attempts(llfe_ctx *ctx, int32_t n, llfe_kmeans_attempt *out);
/* The same diagnostics for any n_colors up to LLFE_MAX_COLORS (k_kmeans and k_kmeans_big), as
 * arrays with k_cap >= n_colors rows per attempt (host): pp_centers and centers
 * [n][10][k_cap][3], counts [n][10][k_cap], iters and compactness [n][10].  Rows past an
 * image's K = min(n_colors, n_unique) are zero.  The same refusals as llfe_kmeans_attempts;
 * k_cap below the launch's n_colors is LLFE_ERR_INVALID. */
int llfe_kmeans_attempts_k(llfe_ctx *ctx, int32_t n, int32_t k_cap, float *pp_centers, float *centers,
                           int32_t *counts, int32_t *iters, double *compactness);
/* Pillow Image.resize(size, LANCZOS, box) on u8 HWC (image_processor.py:221-224).
 * box = (x0, y0, x1, y1) in source pixels, or NULL (whole image); its values are taken at
 * float32 precision, as Pillow takes them. src/dst device. */
int llfe_resize_lanczos_pil(llfe_ctx *ctx, const uint8_t *src, int32_t h, int32_t w, int32_t ch, uint8_t *dst,
                            int32_t out_h, int32_t out_w, const double *box, llfe_stream stream);
/* Pillow Image.reduce((fx, fy)) box averaging of a device u8 HWC image; dst holds
 * ceil(h/fy) x ceil(w/fx) x ch bytes. */
int llfe_reduce_pil(llfe_ctx *ctx, const uint8_t *src, int32_t h, int32_t w, int32_t ch, int32_t fx, int32_t fy,
                    uint8_t *dst, llfe_stream stream);
/* cv2.resize(src, (out_w, out_h), interpolation=...) on a device u8 HWC image (ch <= 4)
 * -- the downscale of validate_and_preprocess_image (app/services/analyze/utils.py:
 * 118-143): LLFE_CV_INTER_AREA for "auto", LLFE_CV_INTER_LANCZOS4 for "high_quality",
 * LLFE_CV_INTER_LINEAR for "performance".  dst holds out_h x out_w x ch bytes. */
#define LLFE_CV_INTER_LINEAR 1
#define LLFE_CV_INTER_CUBIC 2
#define LLFE_CV_INTER_AREA 3
#define LLFE_CV_INTER_LANCZOS4 4
int llfe_resize_cv(llfe_ctx *ctx, const uint8_t *src, int32_t h, int32_t w, int32_t ch, uint8_t *dst, int32_t out_h,
                   int32_t out_w, int32_t interpolation, llfe_stream stream);
/* validate_and_preprocess_image's size rule (utils.py:118-143, Python float
 * semantics): returns 1 with (out_w, out_h, interpolation) when `mode` (LLFE_PRE_*)
 * resizes a w x h image, 0 when it does not. Host only. */
int llfe_preprocess_size(int32_t w, int32_t h, int32_t mode, int32_t *out_w, int32_t *out_h, int32_t *interpolation);
/* PIL Image.thumbnail size rule (preserve_aspect_ratio): returns 1 and the new size
 * when a resize happens, 0 when (w, h) already fits (max_w, max_h). Host only. */
int llfe_thumbnail_size(int32_t w, int32_t h, int32_t max_w, int32_t max_h, int32_t *out_w, int32_t *out_h);
/* ImageProcessor.auto_process_image resize step (image_processor.py:221-224):
 * thumbnail((max_w, max_h), LANCZOS) incl. reducing_gap=2.0's reduce() pre-pass, on a
 * device u8 HWC image.  dst (device) needs out_h * out_w * ch <= dst_capacity bytes. */
int llfe_thumbnail_pil(llfe_ctx *ctx, const uint8_t *src, int32_t h, int32_t w, int32_t ch, int32_t max_w,
                       int32_t max_h, uint8_t *dst, int64_t dst_capacity, int32_t *out_h, int32_t *out_w,
                       llfe_stream stream);
/* the same for n same-size device images packed n x h x w x ch -> n x out_h x out_w x ch
 * (ImageProcessor.auto_process_image over a batch: one launch sequence per pass) */
int llfe_thumbnail_pil_batch(llfe_ctx *ctx, const uint8_t *src, int32_t n, int32_t h, int32_t w, int32_t ch,
                             int32_t max_w, int32_t max_h, uint8_t *dst, int64_t dst_capacity, int32_t *out_h,
                             int32_t *out_w, llfe_stream stream);
/* Image.thumbnail((max_w, max_h), LANCZOS) (reducing_gap 2.0) of a batch whose images each have
 * their own size: where one image's result lies in the packed destination. */
typedef struct {
    int64_t offset;         /* byte offset of this image's result in dst, a multiple of 16 */
    int32_t height, width;  /* result size: llfe_thumbnail_size of the source */
    int32_t resized;        /* 0: the source already fits and is copied */
    int32_t pad_;
} llfe_thumb_out;           /* 24 bytes */
/* host only, no ctx: the layout a call below will write (results in input order, each packed
 * height x width x 3, each starting at a multiple of 16); *dst_bytes = bytes dst must hold (the end
 * of the last result).  LLFE_ERR_INVALID: n < 0, a NULL output, a box side <= 0, or a
 * descriptor llfe_process_images would reject (NULL data, invalid dimensions, a row stride that
 * is neither 0 nor at least 3 * width). */
int llfe_thumbnail_images_layout(const llfe_image_desc *images, int32_t n, int32_t max_w, int32_t max_h,
                                 llfe_thumb_out *outs, int64_t *dst_bytes);
/* ImageProcessor.auto_process_image's resize step over a batch of n BGR u8 images, each its own
 * size, row stride and memory (host or device; the noise fields are ignored), into dst
 * (device), packed as `outs` says (filled as llfe_thumbnail_images_layout fills it).  Every
 * result is byte-identical to llfe_thumbnail_pil of that image.  One plan per distinct size,
 * one upload of all tables, one reduce and one resample launch over all images
 * (thumb_images.hip); device sources are read in place, host sources are staged through a
 * bounded workspace (in chunks when the batch exceeds it; LLFE_THUMB_STAGE_BYTES overrides the
 * bound).  Everything is checked on the host before the first launch: dst_capacity below the
 * layout's total is LLFE_ERR_CAPACITY with dst untouched, a NULL ctx or a bad descriptor
 * LLFE_ERR_INVALID; n == 0 is LLFE_OK.  Synchronous: one stream synchronisation, at the end. */
int llfe_thumbnail_pil_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, int32_t max_w,
                              int32_t max_h, uint8_t *dst, int64_t dst_capacity, llfe_thumb_out *outs,
                              llfe_stream stream);
/* host only: the output tile of the resample kernel (tile_w pixels x at most tile_h rows; the
 * host picks a smaller power-of-two height for an image whose tiles would need more than
 * lds_rows source rows) and the widest filter it takes, so that tests can stand on its seams */
int llfe_thumbnail_images_tiling(int32_t *tile_w, int32_t *tile_h, int32_t *lds_rows, int32_t *max_ksize);
/* validate_and_preprocess_image's resize (utils.py:118-143) of a batch whose images each have
 * their own size: where one image's result lies in the packed destination. */
typedef struct {
    int64_t offset;          /* byte offset of the result in dst, a multiple of 16 */
    int32_t height, width;   /* result size */
    int32_t interpolation;   /* LLFE_CV_INTER_* used; 0 when not resized */
    int32_t resized;         /* 0: the rule leaves it; it is copied */
} llfe_resize_out;           /* 24 bytes */
/* host only, no ctx: the rule (llfe_preprocess_size) per image and the layout a call below will
 * write (results in input order, each packed height x width x 3, each starting at a multiple of
 * 16); *dst_bytes = bytes dst must hold.  LLFE_ERR_INVALID: n < 0, a NULL output, a mode outside
 * LLFE_PRE_*, a descriptor llfe_process_images would reject, or an image whose rule size has a
 * side of 0 (1 x 2001 under LLFE_PRE_AUTO: cv2.resize raises there). */
int llfe_preprocess_images_layout(const llfe_image_desc *images, int32_t n, int32_t preprocessing,
                                  llfe_resize_out *outs, int64_t *dst_bytes);
/* The resize of `preprocessing` over a batch of n BGR u8 images, each its own size, row stride
 * and memory (host or device; the noise fields are ignored), into dst (device), packed as `outs`
 * says (filled as llfe_preprocess_images_layout fills it).  Every result is byte-identical to
 * llfe_resize_cv of that image at the rule's size and interpolation; an image the rule leaves
 * is copied.  One plan per distinct (size, result size, interpolation), one upload of all
 * tables, one launch per plan kind (cvresize_images.hip: k_cv_images_area, _area_fast, _generic,
 * _copy); device sources are read in place, host sources are staged through a bounded workspace
 * of the call's own (in chunks when the batch exceeds it; LLFE_RESIZE_STAGE_BYTES overrides the
 * bound), so the call does not depend on submitted batches.  Everything is checked on the host
 * before the first launch: dst_capacity below the layout's total is LLFE_ERR_CAPACITY with dst
 * untouched; a NULL ctx, a bad descriptor, a bad mode or an image whose rule size has a side of
 * 0 is LLFE_ERR_INVALID (llfe_last_error names the image); n == 0 is LLFE_OK.  Synchronous: one
 * stream synchronisation, at the end. */
int llfe_preprocess_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, int32_t preprocessing,
                           uint8_t *dst, int64_t dst_capacity, llfe_resize_out *outs, llfe_stream stream);
/* The stage entry: sizes3 holds (out_h, out_w, LLFE_CV_INTER_*) per image; every result is
 * byte-identical to llfe_resize_cv(..., 3, out_h, out_w, interpolation).  LINEAR at exactly 2 x 2
 * and AREA upscales run as cv2.resize classifies them; LLFE_CV_INTER_CUBIC is
 * LLFE_ERR_UNSUPPORTED (the text path keeps llfe_resize_cv), any other code or a size <= 0
 * LLFE_ERR_INVALID.  Otherwise as above. */
int llfe_resize_cv_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, const int32_t *sizes3,
                          uint8_t *dst, int64_t dst_capacity, llfe_resize_out *outs, llfe_stream stream);
/* host only: the output tile of the kernels (tile_w pixels x at most tile_h rows; the host picks
 * a smaller power-of-two height for an image whose tiles would need more than lds_rows source
 * rows, and the global-memory arm of the kernel where no height fits), so that tests can stand
 * on its seams */
int llfe_resize_cv_images_tiling(int32_t *tile_w, int32_t *tile_h, int32_t *lds_rows);
/* host-side external contours (findContours RETR_EXTERNAL/CHAIN_APPROX_SIMPLE,
 * shape pyc @L140) on a host u8 mask; points x,y pairs; offsets[n_contours+1].
 * Returns the number of contours, or LLFE_ERR_CAPACITY with *needed_points set. */
int llfe_find_contours(const uint8_t *mask, int32_t h, int32_t w, int32_t *points, int64_t points_capacity,
                       int32_t *offsets, int32_t offsets_capacity, int64_t *needed_points);
/* ShapeAnalyzer.detect_border_radius(contour, epsilon_factor) (shape pyc @L32-61)
 * on one contour (x,y int32 pairs). */
double llfe_border_radius(const int32_t *points, int32_t n, double epsilon_factor);
/* one iteration of the analyze_shapes loop (shape pyc @L146-181): returns 1 and fills
 * *out when contourArea >= 100, 0 when the contour is dropped. */
int llfe_classify_contour(const int32_t *points, int32_t n, llfe_shape *out);
/* host-side shape records from a host u8 mask (the analyze_shapes loop). */
int llfe_shapes_from_mask(const uint8_t *mask, int32_t h, int32_t w, llfe_shape *shapes, int32_t capacity,
                          int32_t *n_contours);
/* The same two on the GPU path the batch uses (contours_gpu.hip: components, border
 * following from first pixels, the raster-scan replay, geometry), from host u8 masks
 * of width <= 4096.  llfe_find_contours_gpu: as llfe_find_contours (cv2 order).
 * llfe_shapes_from_masks_gpu: n masks; per image n_shapes / n_contours, shape records
 * concatenated (LLFE_ERR_CAPACITY with *needed when capacity is short). */
int llfe_find_contours_gpu(llfe_ctx *ctx, const uint8_t *mask, int32_t h, int32_t w, int32_t *points,
                           int64_t points_capacity, int32_t *offsets, int32_t offsets_capacity,
                           int64_t *needed_points);
int llfe_shapes_from_masks_gpu(llfe_ctx *ctx, const uint8_t *masks, int32_t n, int32_t h, int32_t w,
                               llfe_shape *shapes, int64_t capacity, int32_t *n_shapes, int32_t *n_contours,
                               int64_t *needed);

/* ---- host decode (cv2.imdecode(buf, IMREAD_COLOR), utils.py:108-109 and
 * image_processor.py:208-211).  Host only, no ctx.  IMREAD_COLOR semantics: BGR u8.
 * PNG (native decoder): alpha dropped, grey expanded, palette looked up, 16-bit -> high
 * byte, critical-chunk CRCs checked.  JPEG (system libjpeg-turbo via dlopen, OpenCV's
 * settings: ISLOW IDCT, fancy upsampling, JCS_EXT_BGR out).  Images above
 * LLFE_MAX_PIXELS (default 2^30, cv2's CV_IO_MAX_IMAGE_PIXELS) are refused before
 * anything is allocated.  LLFE_ERR_UNSUPPORTED hands an image back to the caller's
 * other decoder: interlaced / sub-byte-depth PNG, CMYK / YCCK JPEG, JPEG with an EXIF
 * orientation other than 1, other formats; corrupt data is LLFE_ERR_INVALID. */
/* size of a PNG from its IHDR; LLFE_ERR_CAPACITY (size still written) above the pixel limit */
int llfe_png_info(const uint8_t *data, uint64_t size, int32_t *width, int32_t *height);
/* n PNGs of one size into out_bgr (n x height x width x 3, host), `threads` host
 * threads.  status[i] per image (LLFE_OK, LLFE_ERR_UNSUPPORTED, LLFE_ERR_INVALID, or
 * LLFE_ERR_CAPACITY when its size differs); returns the first non-OK status. */
int llfe_decode_png_batch(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height,
                          int32_t width, uint8_t *out_bgr, int32_t *status, int32_t threads);
/* the same two for PNG and JPEG, by signature (LLFE_ERR_UNSUPPORTED for other formats) */
int llfe_image_info(const uint8_t *data, uint64_t size, int32_t *width, int32_t *height);
int llfe_decode_batch(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height, int32_t width,
                      uint8_t *out_bgr, int32_t *status, int32_t threads);
/* which codecs the host decoders run: "png=libdeflate|zlib;jpeg=libjpeg.so.8|pillow"
 * (NUL-terminated into buf; LLFE_ERR_CAPACITY if cap is too small) */
int llfe_decoder_info(char *buf, int32_t cap);

/* ---- JPEG decode split in two (the same cv2.imdecode(buf, IMREAD_COLOR) at utils.py:108-109
 * and image_processor.py:208-211): the host does the entropy half (libjpeg-turbo's
 * jpeg_read_coefficients), the device the reconstruction -- dequantisation, ISLOW inverse
 * DCT, fancy chroma upsampling, YCbCr -> BGR -- bit for bit what llfe_decode_batch writes.
 * Opt-in; llfe_decode_batch is unchanged.
 *
 * A batch of one image size is staged in slots of one stride.  Image i's slot holds its
 * components' 64 x u16 quantisation tables (natural order) and their quantised
 * coefficients: blocks_h rows of blocks_w blocks, a block 64 x int16 in natural order.
 * llfe_jpeg_desc says where (byte offsets inside the slot). */
#define LLFE_JPEG_GRAY 1 /* one component, replicated to B, G, R */
#define LLFE_JPEG_444 2  /* YCbCr, luma sampled 1x1 */
#define LLFE_JPEG_422 3  /* luma 2x1: chroma at half width (h2v1 fancy upsampling) */
#define LLFE_JPEG_420 4  /* luma 2x2: chroma at half width and height (h2v2 fancy upsampling) */
typedef struct {
    int32_t n_comp;   /* 1 or 3; 0: nothing staged (the image was not eligible), reconstruction skips it */
    int32_t sampling; /* LLFE_JPEG_* */
    struct {
        int32_t blocks_w, blocks_h; /* width_in_blocks, height_in_blocks */
        int32_t width, height;      /* downsampled_width, downsampled_height: the component's real samples */
        int64_t coef_offset;        /* blocks_h * blocks_w * 128 bytes, 16-byte aligned */
        int64_t quant_offset;       /* 128 bytes, 16-byte aligned */
    } comp[3];
} llfe_jpeg_desc; /* 104 bytes */
/* host only: bytes of a slot that holds any eligible height x width image (4:4:4, the
 * worst case; a multiple of 128); LLFE_ERR_INVALID for sizes outside 1..65535 */
int64_t llfe_jpeg_coef_slot_bytes(int32_t height, int32_t width);
/* host only, no ctx: entropy-decode n JPEGs of one size on `threads` host threads into
 * slots (host, n x slot_stride bytes) and descs[n].  slot_stride = llfe_jpeg_coef_slot_bytes
 * holds every eligible image; with a smaller one (a 4:2:0 feed needs half) an image that
 * does not fit is LLFE_ERR_UNSUPPORTED like any other this path hands back.
 * status[i] per image; returns the first non-OK status, like llfe_decode_batch.  Eligible:
 * 8-bit, greyscale or YCbCr with chroma 1x1 and luma 1x1 / 2x1 / 2x2, EXIF orientation 1 (or
 * 2 .. 8 under LLFE_JPEG_ORIENT, which only the mixed-size entry points below take),
 * no libjpeg warning (a truncated scan is one), every progressive scan present; baseline,
 * progressive, optimised-Huffman, restart-interval and arithmetic files alike.  Anything
 * else (other formats included) is LLFE_ERR_UNSUPPORTED, or when this libjpeg lacks
 * jpeg_read_coefficients: decode it with llfe_decode_batch.  Corrupt data is
 * LLFE_ERR_INVALID, another size LLFE_ERR_CAPACITY.  A non-OK image's slot is not written
 * and its descs[i].n_comp is 0. */
int llfe_jpeg_read_coefs_batch(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height,
                               int32_t width, uint8_t *slots, int64_t slot_stride, llfe_jpeg_desc *descs,
                               int32_t *status, int32_t threads);
/* the device half: coefs (device, n x slot_stride bytes, 16-byte aligned, as staged above)
 * -> out_bgr (device, n x h x w x 3 u8).  descs is a host array and is validated on the
 * host before anything is launched: every offset and extent inside the slot, the block
 * grids covering h x w at the sampling class; a bad descriptor is LLFE_ERR_INVALID with
 * out_bgr untouched.  Images with n_comp == 0 are left as they are in out_bgr (the caller
 * fills them from llfe_decode_batch).  The same kernel as llfe_jpeg_reconstruct_images below,
 * one launch over the (image, tile) pairs of the call: no workspace and no chunks; more than
 * 2^31 tiles in one call are LLFE_ERR_CAPACITY.  Runs on `stream` and returns when it has
 * finished. */
int llfe_jpeg_reconstruct(llfe_ctx *ctx, const uint8_t *coefs, int64_t slot_stride, const llfe_jpeg_desc *descs,
                          int32_t n, int32_t h, int32_t w, uint8_t *out_bgr, llfe_stream stream);

/* ---- the same split decode for a batch whose images each have their own size (opt-in): the
 * coefficient slots are tight and lie one behind the other in one staging buffer, the results
 * are packed height x width x 3 where the caller says, and one launch of csrc/jpeg_images.hip
 * reconstructs every image, whatever its size and sampling class, bit for bit what
 * llfe_decode_batch writes.  llfe_jpeg_image says where one image's slot and result lie. */
typedef struct {
    int64_t slot_offset;   /* of this image's coefficient slot in the staged buffer, 16-byte aligned */
    int64_t slot_bytes;    /* room in that slot, a multiple of 16; 0: nothing staged */
    int64_t out_offset;    /* of this image's height x width x 3 BGR result in `out`, a multiple of 16 */
    int32_t height, width;
} llfe_jpeg_image;         /* 32 bytes */
/* host only, no ctx, headers only: images[n] for n blobs.  A JPEG that is eligible as far as its
 * header tells (what llfe_jpeg_read_coefs_batch takes) gets its height and width, a tight
 * slot_bytes (the end of its last component as llfe_jpeg_read_coefs_batch lays a slot out,
 * rounded up to 16: a 4:2:0 file takes half a 4:4:4 slot) and slot_offset, the running sum;
 * *slots_bytes receives the total.  Any other image keeps slot_bytes = 0 and gets
 * LLFE_ERR_UNSUPPORTED (PNG, CMYK, an EXIF orientation other than 1 unless LLFE_JPEG_ORIENT, other
 * samplings, 12-bit files, other formats), LLFE_ERR_INVALID (corrupt data, a NULL blob) or LLFE_ERR_CAPACITY (a
 * size above LLFE_MAX_PIXELS, as llfe_image_info); its size is still written when the header
 * gave one, else 0 x 0.  out_offset is not touched: the caller lays out the output, because it
 * knows the sizes of the images its other decoder takes.  status[i] per image; returns the
 * first non-OK status. */
int llfe_jpeg_images_layout(const uint8_t *const *data, const uint64_t *sizes, int32_t n, llfe_jpeg_image *images,
                            int64_t *slots_bytes, int32_t *status, int32_t threads);
/* EXIF orientation on the device (opt-in).  The flag is the same bit in every flags word of the
 * mixed-size entry points; any other bit there is LLFE_ERR_INVALID, and so is this one in the
 * same-size entry points (llfe_jpeg_parse_batch_flags).  With it a JPEG whose EXIF orientation
 * (tag 0x0112 of IFD0) is 2 .. 8 is eligible like the same file without EXIF: its slot, its
 * descriptor and its record are byte for byte that file's, llfe_jpeg_image.height / width stay
 * the coded size, and the orientation travels beside the records as one byte per image.
 * llfe_jpeg_reconstruct_images_oriented then writes the result Pillow's
 * ImageOps.exif_transpose gives (csrc/jpeg_orient.h holds the map): height x width for 1 .. 4,
 * width x height for 5 .. 8.  A tag value outside 1 .. 8 keeps LLFE_ERR_UNSUPPORTED. */
#define LLFE_JPEG_ORIENT 4u
/* llfe_jpeg_images_layout with flags.  orientation (n bytes; may be NULL without
 * LLFE_JPEG_ORIENT) receives 1 for every image, and with LLFE_JPEG_ORIENT the EXIF orientation
 * 2 .. 8 of an eligible JPEG that has one.  flags = 0 is llfe_jpeg_images_layout. */
int llfe_jpeg_images_layout_flags(const uint8_t *const *data, const uint64_t *sizes, int32_t n, llfe_jpeg_image *images,
                                  int64_t *slots_bytes, int32_t *status, int32_t threads, uint8_t *orientation,
                                  uint32_t flags);
/* host only: the CPU twin of the orientation store of csrc/jpeg_images.hip.  src_bgr (h x w x 3)
 * -> dst_bgr (h x w x 3 for orientation 1 .. 4, w x h x 3 for 5 .. 8) through the map of
 * csrc/jpeg_orient.h; LLFE_ERR_INVALID for an orientation outside 1 .. 8, a NULL pointer or a
 * size below 1. */
int llfe_jpeg_orient_reference(const uint8_t *src_bgr, int32_t h, int32_t w, int32_t orientation, uint8_t *dst_bgr);
/* host only, no ctx: llfe_jpeg_read_coefs_batch with each image's own height, width and slot
 * (images[i], as laid out above) in slots (host, slots_bytes bytes).  The llfe_jpeg_desc offsets
 * stay relative to the image's slot.  status[i] as llfe_jpeg_read_coefs_batch's: an image that
 * does not fit its slot_bytes is LLFE_ERR_UNSUPPORTED with n_comp = 0, another size than its
 * record says LLFE_ERR_CAPACITY; slot_bytes == 0 is LLFE_ERR_UNSUPPORTED and nothing is read.
 * A slot outside slots_bytes (or one not 16-byte aligned) is LLFE_ERR_INVALID for the whole
 * call, before any decode.  Returns the first non-OK status. */
int llfe_jpeg_read_coefs_images(const uint8_t *const *data, const uint64_t *sizes, int32_t n,
                                const llfe_jpeg_image *images, uint8_t *slots, int64_t slots_bytes,
                                llfe_jpeg_desc *descs, int32_t *status, int32_t threads);
/* the same with flags: LLFE_JPEG_ORIENT takes files with an EXIF orientation 2 .. 8 as well and
 * changes nothing else; any other bit is LLFE_ERR_INVALID */
int llfe_jpeg_read_coefs_images_flags(const uint8_t *const *data, const uint64_t *sizes, int32_t n,
                                      const llfe_jpeg_image *images, uint8_t *slots, int64_t slots_bytes,
                                      llfe_jpeg_desc *descs, int32_t *status, int32_t threads, uint32_t flags);
/* the device half: coefs (device, coefs_bytes bytes, 16-byte aligned, as staged above) -> out
 * (device, out_capacity bytes), image i packed height x width x 3 at images[i].out_offset.
 * images and descs are host arrays, validated on the host before anything is launched; for
 * every image with n_comp != 0: its descriptor against its own height x width and slot_bytes
 * (as llfe_jpeg_reconstruct checks one), its slot inside coefs_bytes, out_offset a multiple of
 * 16, its result inside out_capacity and apart from every other image's.  A bad record is
 * LLFE_ERR_INVALID, or LLFE_ERR_CAPACITY when only out_capacity is short; out is untouched in
 * both cases.  Images with n_comp == 0 are skipped, their records are not read and their
 * places in out stay as they are.  Runs on `stream` and returns when it has finished. */
int llfe_jpeg_reconstruct_images(llfe_ctx *ctx, const uint8_t *coefs, int64_t coefs_bytes, const llfe_jpeg_image *images,
                                 const llfe_jpeg_desc *descs, int32_t n, uint8_t *out, int64_t out_capacity,
                                 llfe_stream stream);
/* the same with an EXIF orientation per image (host array of n bytes, 1 .. 8; NULL: all 1, which
 * is llfe_jpeg_reconstruct_images): image i's result at images[i].out_offset is the coded
 * height x width raster re-indexed as csrc/jpeg_orient.h says, packed height x width x 3 for
 * 1 .. 4 and width x height x 3 for 5 .. 8 -- the same height * width * 3 bytes, which is what the
 * overlap and capacity checks count.  An orientation outside 1 .. 8 of an image with n_comp != 0
 * is LLFE_ERR_INVALID with out untouched.  The images are reconstructed by orientation group
 * (1; 2 .. 4; 5 .. 8), at most three launches. */
int llfe_jpeg_reconstruct_images_oriented(llfe_ctx *ctx, const uint8_t *coefs, int64_t coefs_bytes,
                                          const llfe_jpeg_image *images, const llfe_jpeg_desc *descs,
                                          const uint8_t *orientation, int32_t n, uint8_t *out, int64_t out_capacity,
                                          llfe_stream stream);
/* host only: the output tile of csrc/jpeg_images.hip for a sampling class (LLFE_JPEG_*), a
 * multiple of the class's MCU, so that tests can stand on its seams; LLFE_ERR_INVALID for an
 * unknown class */
int llfe_jpeg_images_tiling(int32_t sampling, int32_t *tile_w, int32_t *tile_h);

/* ---- the entropy half on the device too (opt-in): baseline sequential Huffman files with one
 * interleaved scan, without restart markers or (llfe_jpeg_parse_batch_flags) with them.  The host only parses the headers; the file's scan
 * bytes cross to the device instead of its coefficients, csrc/jpeg_huff.hip writes exactly the
 * coefficient slots llfe_jpeg_read_coefs_batch writes, and llfe_jpeg_reconstruct runs on them
 * unchanged.
 *
 * A batch is staged as one record per image in a buffer of one record stride:
 *   quant_offset   n_comp x 64 u16 quantisation tables, natural order
 *   table_offset   four decode tables (DC 0, DC 1, AC 0, AC 1) of LLFE_JPEG_HUFF_TABLE_BYTES:
 *                  u32 lim[18], i32 off[18], u8 vals[256] (csrc/jpeg_huff_core.h)
 *   scan_offset    the scan's entropy-coded bytes as they are in the file (stuffed FF 00 pairs
 *                  and restart markers included), zero padded to a multiple of 16 plus 16
 * llfe_jpeg_scan (a host array, like llfe_jpeg_desc) says where, and carries the MCU geometry. */
#define LLFE_JPEG_HUFF_TABLE_BYTES 400
#define LLFE_JPEG_RECORD_HEADER 2048 /* bytes of a record in front of its scan bytes */
typedef struct {
    int64_t record_offset; /* of the image's record in the staging buffer, 16-byte aligned */
    int32_t quant_offset, table_offset, scan_offset; /* inside the record, 16-byte aligned */
    int32_t scan_bytes;           /* up to (excluding) the EOI marker */
    int32_t mcus_w, mcus_h;       /* the MCU grid of the scan */
    int32_t blocks_in_mcu;        /* 1..6; 0: nothing staged */
    uint8_t blk_comp[8];          /* per block of one MCU: its component, */
    uint8_t blk_x[8], blk_y[8];   /*   its place inside the MCU in blocks, */
    uint8_t blk_dc[8], blk_ac[8]; /*   its DC and AC table (0 or 1) */
    uint8_t comp_hs[4], comp_vs[4]; /* per component: blocks per MCU across and down */
    int32_t restart_interval;     /* MCUs between restart markers (the file's DRI), 0..65535; 0: none */
} llfe_jpeg_scan; /* 88 bytes */
/* host only, no ctx: the host half.  Parses n blobs of one size on `threads` host threads into
 * staging (host, n x record_stride bytes; record_stride a multiple of 16, at least
 * LLFE_JPEG_RECORD_HEADER + the longest blob rounded up to 16 + 16 holds any), descs[n] (the
 * geometry and slot offsets llfe_jpeg_read_coefs_batch computes, for slots of slot_stride
 * bytes) and scans[n].  Eligible: what llfe_jpeg_read_coefs_batch takes (the colour space,
 * precision and sampling decisions are libjpeg's jpeg_read_header), and on top of that SOF0 /
 * SOF1 Huffman, 8-bit, exactly one SOS with all components in frame order and Ss = 0,
 * Se = 63, Ah = Al = 0, table ids 0 or 1, no restart interval, every referenced DHT present
 * and a valid prefix code, and the scan ending at an FF D9 that is the first marker after it.
 * Anything else is LLFE_ERR_UNSUPPORTED (progressive, arithmetic, restart intervals,
 * multi-scan, EXIF orientation != 1 unless LLFE_JPEG_ORIENT (llfe_jpeg_parse_images only), CMYK,
 * other formats): nothing is written for it,
 * descs[i].n_comp and scans[i].blocks_in_mcu are 0, and it takes llfe_jpeg_read_coefs_batch
 * or llfe_decode_batch.  status[i] per image; returns the first non-OK status.  This is
 * llfe_jpeg_parse_batch_flags with flags = 0: every record it stages has restart_interval 0. */
int llfe_jpeg_parse_batch(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height, int32_t width,
                          uint8_t *staging, int64_t record_stride, int64_t slot_stride, llfe_jpeg_desc *descs,
                          llfe_jpeg_scan *scans, int32_t *status, int32_t threads);
/* The same with flags (any other bit is LLFE_ERR_INVALID).  LLFE_JPEG_PARSE_RESTARTS: files with
 * a restart interval (a DRI of 1..65535, the value libjpeg's jpeg_read_header reports) are
 * eligible as well.  Inside the scan of such a file an FF is followed by 00, by D0..D7, or by the
 * terminating D9; FF FF fill bytes and every other marker stay LLFE_ERR_UNSUPPORTED.  The scan
 * is staged raw, markers included, and scans[i].restart_interval holds the DRI.  The parser does
 * not decode: whether the markers stand where the interval says is decided by
 * llfe_jpeg_entropy_decode / llfe_jpeg_entropy_reference, which hand the image back if not.  A
 * DRI of 0, or one no marker follows because it is not below the MCU count, is a restart-free
 * scan. */
#define LLFE_JPEG_PARSE_RESTARTS 1u
int llfe_jpeg_parse_batch_flags(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height,
                                int32_t width, uint8_t *staging, int64_t record_stride, int64_t slot_stride,
                                llfe_jpeg_desc *descs, llfe_jpeg_scan *scans, int32_t *status, int32_t threads,
                                uint32_t flags);
/* host only: the plain C++ twin of llfe_jpeg_entropy_decode over host memory (staging and
 * slots on the host), for tests and for debugging the kernels: the same subsequences, rounds,
 * verification, block scan, write pass and DC sums, run serially.  one_piece != 0: decode each
 * scan from its first bit to its last in one piece instead.  The same validation; status[i]:
 * LLFE_OK, or LLFE_ERR_UNSUPPORTED for an image that was not staged or whose scan shows an
 * anomaly, misplaced restart markers (below) included. */
int llfe_jpeg_entropy_reference(const uint8_t *staging, int64_t staging_bytes, const llfe_jpeg_scan *scans,
                                const llfe_jpeg_desc *descs, int32_t n, int32_t h, int32_t w, uint8_t *slots,
                                int64_t slot_stride, int32_t *status, int32_t one_piece);
/* the device half: staging (device, staging_bytes, 16-byte aligned, as parsed above) -> slots
 * (device, n x slot_stride).  scans and descs are host arrays and are validated on the host
 * before anything is launched: every record, table and scan extent inside staging_bytes,
 * every descriptor inside its slot (as llfe_jpeg_reconstruct checks it), the MCU geometry
 * covering the block grids, restart_interval in 0..65535; a bad one is LLFE_ERR_INVALID with the slots untouched.  Images
 * with blocks_in_mcu == 0 are skipped.  The kernels read nothing outside what was validated
 * (the bit reader is bounded by scan_bytes) and every loop has a bound fixed on the host.
 * status_out (host, n): LLFE_OK for an image whose slot now holds its quantisation tables and
 * coefficients, LLFE_ERR_UNSUPPORTED for one that was skipped or whose scan showed an anomaly
 * (no such code, a coefficient index past 63, a DC category above 11 or an AC category above
 * 10, the scan not ending inside its last byte, leftover bits that are not 1-padding, a block
 * count other than the frame's, the verification of the subsequence states failing; with a
 * restart interval Ri also: a marker met anywhere but at an MCU boundary behind 0..7 one-bits,
 * the k-th marker (k = 0, 1, ...) not FF D0 + (k & 7) or not behind exactly (k + 1) * Ri MCUs,
 * two adjacent markers, a marker behind the last MCU, a marker missing): its slot
 * may hold anything and the caller decodes it another way.  Runs on `stream` and returns when
 * it has finished. */
int llfe_jpeg_entropy_decode(llfe_ctx *ctx, const uint8_t *staging, int64_t staging_bytes, const llfe_jpeg_scan *scans,
                             const llfe_jpeg_desc *descs, int32_t n, int32_t h, int32_t w, uint8_t *slots,
                             int64_t slot_stride, int32_t *status_out, llfe_stream stream);

/* ---- the device entropy decode for a batch whose images each have their own size (opt-in): the
 * records lie one behind the other in one staging buffer, each as long as its file needs, and
 * csrc/jpeg_huff.hip writes the tight slots llfe_jpeg_read_coefs_images writes, for
 * llfe_jpeg_reconstruct_images to run on unchanged. */
/* host only, no ctx: where the records go.  For every image whose images[i].slot_bytes != 0 (as
 * llfe_jpeg_images_layout left it) record_offsets[i] is the running sum and the record takes
 * LLFE_JPEG_RECORD_HEADER + sizes[i] rounded up to 16 + 16 bytes; the other images take no room
 * (their offset is the running sum too).  *staging_bytes receives the total.  Returns LLFE_OK, or
 * LLFE_ERR_INVALID for a NULL argument or a negative n. */
int llfe_jpeg_records_layout(const uint64_t *sizes, const llfe_jpeg_image *images, int32_t n, int64_t *record_offsets,
                             int64_t *staging_bytes);
/* host only, no ctx: llfe_jpeg_parse_batch_flags with each image's own height, width and
 * slot_bytes (images[i]) and its record at record_offsets[i] in staging (host, staging_bytes
 * bytes).  The llfe_jpeg_desc offsets are relative to the image's tight slot: byte for byte the
 * descriptor llfe_jpeg_read_coefs_images produces for the file.  The same eligibility rules and
 * the same flags, and LLFE_JPEG_ORIENT on top (files with an EXIF orientation 2 .. 8 are taken
 * and staged as the same file without EXIF).  status[i] as llfe_jpeg_parse_batch's: a file that does not fit its slot_bytes
 * is LLFE_ERR_UNSUPPORTED, another size than its record says LLFE_ERR_CAPACITY; slot_bytes == 0
 * is LLFE_ERR_UNSUPPORTED and nothing is read.  A record (as llfe_jpeg_records_layout sizes it)
 * outside staging_bytes, or one not 16-byte aligned, is LLFE_ERR_INVALID for the whole call,
 * before any parse.  Returns the first non-OK status. */
int llfe_jpeg_parse_images(const uint8_t *const *data, const uint64_t *sizes, int32_t n, const llfe_jpeg_image *images,
                           const int64_t *record_offsets, uint8_t *staging, int64_t staging_bytes,
                           llfe_jpeg_desc *descs, llfe_jpeg_scan *scans, int32_t *status, int32_t threads,
                           uint32_t flags);
/* host only: llfe_jpeg_entropy_reference over tight slots (slots on the host, slots_bytes bytes,
 * image i at images[i].slot_offset); the validation of llfe_jpeg_entropy_decode_images. */
int llfe_jpeg_entropy_reference_images(const uint8_t *staging, int64_t staging_bytes, const llfe_jpeg_scan *scans,
                                       const llfe_jpeg_desc *descs, const llfe_jpeg_image *images, int32_t n,
                                       uint8_t *slots, int64_t slots_bytes, int32_t *status, int32_t one_piece);
/* the device half: staging (device, staging_bytes, 16-byte aligned, as parsed above) -> slots
 * (device, slots_bytes, 16-byte aligned).  scans, descs and images are host arrays, validated on
 * the host before anything is launched; for every image with blocks_in_mcu != 0: its descriptor
 * against its own height x width and slot_bytes, its slot 16-byte aligned, inside slots_bytes and
 * apart from every other such image's, its record as llfe_jpeg_entropy_decode checks one.  A bad
 * record is LLFE_ERR_INVALID with the slots untouched; more than 2^31 subsequences or blocks in
 * one call is LLFE_ERR_CAPACITY.  status_out as llfe_jpeg_entropy_decode's; for an image the
 * device does not take the slot may hold anything, but only its own slot.  Runs on `stream` and
 * returns when it has finished. */
int llfe_jpeg_entropy_decode_images(llfe_ctx *ctx, const uint8_t *staging, int64_t staging_bytes,
                                    const llfe_jpeg_scan *scans, const llfe_jpeg_desc *descs,
                                    const llfe_jpeg_image *images, int32_t n, uint8_t *slots, int64_t slots_bytes,
                                    int32_t *status_out, llfe_stream stream);

/* ---- PNG decode on the device (opt-in; llfe_decode_batch is unchanged): 8-bit RGB / RGBA,
 * not interlaced.  The host only walks the chunks; the file's deflate stream crosses to the
 * device instead of its pixels, and csrc/png_inflate.hip inflates, checks the Adler-32, undoes
 * the row filters and writes the BGR batch, bit for bit what llfe_decode_batch writes.
 *
 * A batch is staged as one record per image in a buffer of one record stride: the IDAT
 * payloads concatenated (zero-length and 1-byte chunks included) without the two zlib header
 * bytes and the four Adler-32 bytes, zero padded to a multiple of 16, then 16 zero bytes, then
 * the stored Adler-32 (u32) and 12 zero bytes.  llfe_png_desc (a host array) says where. */
typedef struct {
    int64_t record_offset; /* of the image's record in the staging buffer, 16-byte aligned */
    int64_t raw_bytes;     /* height * (row_bytes + 1): what the stream must inflate to */
    int32_t deflate_bytes; /* bytes of the deflate stream; 0: nothing staged */
    int32_t bpp;           /* bytes per pixel: 3 (RGB) or 4 (RGBA) */
    int32_t row_bytes;     /* width * bpp */
    uint32_t adler;        /* the Adler-32 the file stores */
} llfe_png_desc; /* 32 bytes */
/* host only, no ctx: the host half.  Walks the chunks of n blobs of one size on `threads` host
 * threads (critical-chunk CRCs checked, LLFE_MAX_PIXELS applied, as llfe_decode_batch does) and
 * stages the eligible ones into staging (host, n x record_stride bytes; record_stride a multiple
 * of 16, the longest blob rounded up to 16 plus 32 holds any) and descs[n].  Eligible: colour
 * type 2 or 6 at 8 bits, not interlaced, of the batch's size, a zlib header with CM = 8,
 * CINFO <= 7, no FDICT and a valid FCHECK, raw_bytes below 2^31 and plausible for the IDAT
 * bytes, the record fitting record_stride.  Everything else (grey, palette, 16-bit, sub-byte,
 * interlaced, JPEG, other formats, another size) keeps a zeroed descriptor and is
 * LLFE_ERR_UNSUPPORTED; a corrupt container is LLFE_ERR_INVALID as in llfe_decode_batch.
 * Decode those with llfe_decode_batch.  status[i] per image; returns the first non-OK status. */
int llfe_png_parse_batch(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height, int32_t width,
                         uint8_t *staging, int64_t record_stride, llfe_png_desc *descs, int32_t *status,
                         int32_t threads);
/* host only: the plain C++ twin of llfe_png_decode_device over host memory, built from the same
 * decoding core (csrc/png_inflate_core.h), for tests and for debugging the kernels.  raw (n x
 * raw_stride) receives the inflated filtered rows, out_bgr (n x h x w x 3) the pixels.  The same
 * validation; status[i]: LLFE_OK, or LLFE_ERR_UNSUPPORTED for an image that was not staged or
 * whose stream shows an anomaly (below). */
int llfe_png_decode_reference(const uint8_t *staging, int64_t staging_bytes, const llfe_png_desc *descs, int32_t n,
                              int32_t h, int32_t w, uint8_t *raw, int64_t raw_stride, uint8_t *out_bgr,
                              int32_t *status);
/* the device half: staging (device, staging_bytes, 16-byte aligned, as parsed above) -> raw
 * (device, n x raw_stride, 16-byte aligned, raw_stride a multiple of 16 and at least raw_bytes:
 * the inflated filtered rows) and out_bgr (device, n x h x w x 3).  descs is a host array and is
 * validated on the host before anything is launched: every record inside staging_bytes, the
 * geometry h x w at 3 or 4 bytes per pixel; a bad one is LLFE_ERR_INVALID with nothing written
 * (so is n above 65535).
 * Images with deflate_bytes == 0 are skipped and left as they are in out_bgr.  status (host, n):
 * LLFE_OK for an image whose pixels are in out_bgr, LLFE_ERR_UNSUPPORTED for one that was
 * skipped or whose stream showed an anomaly: reserved block type 3, a stored block whose NLEN
 * is not ~LEN, a set of code lengths that is over-subscribed or incomplete (other than a
 * single code of length 1, or no distance code), a dynamic header zlib refuses, no such code,
 * length symbols 286 / 287 or distance codes 30 / 31, a distance beyond the bytes produced so
 * far, output that would pass raw_bytes, input exhausted before the final block's end, the
 * final block ending before raw_bytes, a filter byte above 4, an Adler-32 mismatch.  Its raw
 * and pixels may hold anything and the caller decodes it with llfe_decode_batch.  The kernels
 * read nothing outside the validated records and every loop is bounded by the record.  Runs
 * on `stream` and returns when it has finished. */
int llfe_png_decode_device(llfe_ctx *ctx, const uint8_t *staging_dev, int64_t staging_bytes,
                           const llfe_png_desc *descs, int32_t n, int32_t h, int32_t w, uint8_t *raw_dev,
                           int64_t raw_stride, uint8_t *out_bgr_dev, int32_t *status, llfe_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* LLFE_H */
