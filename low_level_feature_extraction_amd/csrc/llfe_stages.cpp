// C ABI of libllfe.so (include/llfe.h): the stage drop-ins -- single stages of the pipeline
// (stencil, hysteresis, unique colours, k-means, contours, fonts) on lane 0's workspace,
// host slot 0's buffers and the caller's stream, and the host-only contour services.
#include "llfe_ctx.h"

using namespace llfe_host;

namespace {

int font_bits_stage(llfe_ctx *ctx, const uint8_t *bgr, const uint64_t *img_tab, uint64_t *bits, int n, int h, int w,
                    hipStream_t s) {
    TIMED(ctx, s, "k_font_bits", (double)n * h * w * (3 + 0.125), launch_font_bits(bgr, img_tab, n, h, w, bits, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->prof.collect(-2);
    return LLFE_OK;
}

// host u8 masks -> bit-packed on the device -> GPU contour pass on lane 0 (synchronous;
// capacities grown until nothing overflows).  Leaves the results in W.d_ct_* and
// host slot 0's copies.
int gpu_contours_of_masks(llfe_ctx *ctx, const uint8_t *masks, int n, int h, int w) {
    if (w > kCtMaxWidth || h > kCtMaxHeight)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "GPU contours need width <= %d and height <= %d", kCtMaxWidth,
                         kCtMaxHeight);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    Work &W = ctx->lanes[0].W;
    HostSlot &H = ctx->slots[0];
    hipStream_t s = ctx->lanes[0].stream;
    const int wpr = words_per_row(w);
    std::vector<uint64_t> bits((size_t)n * h * wpr, 0ull);
    for (size_t r = 0; r < (size_t)n * h; r++)
        for (int x = 0; x < w; x++)
            if (masks[r * w + x]) bits[r * wpr + (x >> 6)] |= 1ull << (x & 63);
    HIPCHK(ctx, W.d_bits.ensure(bits.size()));
    HIPCHK(ctx, hipMemcpyAsync(W.d_bits.p, bits.data(), sizeof(uint64_t) * bits.size(), hipMemcpyHostToDevice, s));
    for (int attempt = 0;; attempt++) {
        int rc = run_contours(ctx, W, n, h, w, W.d_bits.p, s);
        if (rc) return rc;
        rc = copy_contours(ctx, W, n, H, s);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(s));
        const CtCounters ct = *H.h_ct_ctr.p;
        if (ct.flags & (kCtBadTrace | kCtTooWide | kCtDpOverflow))
            return ctx->fail(LLFE_ERR_UNSUPPORTED, "GPU contours: unsupported mask (flags 0x%x)", ct.flags);
        if (!(ct.flags & kCtOverflowMask)) return LLFE_OK;
        if (attempt >= 8) return ctx->fail(LLFE_ERR_CAPACITY, "GPU contours: capacities still overflow");
        grow_contour_caps(W, n, h, w, ct);
    }
}

}  // namespace

extern "C" {

int llfe_gray_blur5(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *blurred, int32_t n, int32_t h, int32_t w,
                    llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || !bgr || !blurred) return LLFE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_stencil(bgr, n, h, w, nullptr, blurred, nullptr, nullptr, nullptr, ctx->sp, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    return LLFE_OK;
}

int llfe_edge_classes(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *classes, int32_t n, int32_t h, int32_t w,
                      llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || !bgr || !classes) return LLFE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_stencil(bgr, n, h, w, classes, nullptr, nullptr, nullptr, nullptr, ctx->sp, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    return LLFE_OK;
}

int llfe_font_binary(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *mask, int32_t n, int32_t h, int32_t w,
                     llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || !bgr || !mask) return LLFE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_font_binary(bgr, n, h, w, mask, ctx->sp, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    return LLFE_OK;
}

int llfe_font_bits(llfe_ctx *ctx, const uint8_t *bgr, uint64_t *bits, int32_t n, int32_t h, int32_t w,
                   llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || !bgr || !bits) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return font_bits_stage(ctx, bgr, nullptr, bits, n, h, w, (hipStream_t)stream);
}

int llfe_font_bits_images(llfe_ctx *ctx, const uint8_t *const *images, uint64_t *bits, int32_t n, int32_t h,
                          int32_t w, llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || n < 1 || !images || !bits) return LLFE_ERR_INVALID;
    for (int i = 0; i < n; i++)
        if (!images[i]) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    HostSlot &H = ctx->slots[0];  // (host slot 0's gather table: no batch is in flight)
    HIPCHK(ctx, H.h_gather.ensure((size_t)n));
    HIPCHK(ctx, H.d_gather.ensure((size_t)n));
    for (int i = 0; i < n; i++) H.h_gather.p[i] = (uint64_t)(uintptr_t)images[i];
    HIPCHK(ctx, hipMemcpyAsync(H.d_gather.p, H.h_gather.p, sizeof(uint64_t) * n, hipMemcpyHostToDevice, s));
    return font_bits_stage(ctx, images[0], H.d_gather.p, bits, n, h, w, s);
}

int llfe_font_bits_tiling(int32_t h, int32_t w, int32_t *strip_w, int32_t *seg_h) {
    if (!valid_dims(1, h, w) || !strip_w || !seg_h) return LLFE_ERR_INVALID;
    int strips, segs, rows;
    font_bits_tiling(h, w, &strips, &segs, &rows);
    *strip_w = font_bits_strip_width();
    *seg_h = rows;
    return LLFE_OK;
}

int llfe_shape_mask(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *mask, int32_t n, int32_t h, int32_t w,
                    llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || !bgr || !mask) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    Work &W = ctx->lanes[0].W;  // stage entry points run on the caller's stream, lane 0's workspace
    HIPCHK(ctx, W.d_cls.ensure((size_t)n * h * w));
    StencilParams sp;
    int rc = stencil_params(ctx, W, n, h, w, s, &sp);
    if (rc) return rc;
    HIPCHK(ctx, launch_stencil(bgr, n, h, w, W.d_cls.p, nullptr, nullptr, nullptr, nullptr, sp, s));
    rc = run_hysteresis_dilate(ctx, W, n, h, w, nullptr, mask, s);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->prof.collect(-2);
    return LLFE_OK;
}

// Canny(blur5(gray), 50, 150) of the shapes path (shape pyc @L6-30) before the
// dilation: the stencil's edge classes, then the hysteresis components, as 0 / 255
int llfe_canny(llfe_ctx *ctx, const uint8_t *bgr, uint8_t *edges, int32_t n, int32_t h, int32_t w,
               llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || !bgr || !edges) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    Work &W = ctx->lanes[0].W;
    HIPCHK(ctx, W.d_cls.ensure((size_t)n * h * w));
    StencilParams sp;
    int rc = stencil_params(ctx, W, n, h, w, s, &sp);
    if (rc) return rc;
    HIPCHK(ctx, launch_stencil(bgr, n, h, w, W.d_cls.p, nullptr, nullptr, nullptr, nullptr, sp, s));
    HystWork wk;
    rc = hyst_work(ctx, W, n, h, w, &wk);
    if (rc) return rc;
    HIPCHK(ctx, launch_canny_edges(W.d_cls.p, n, h, w, wk, edges, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return LLFE_OK;
}

// The hysteresis of llfe_canny / llfe_shape_mask on a caller's class maps (host in / out,
// lane 0, synchronous).  The kernels' 16-byte and bytewise row readers agree only on
// bytes 0 / 1 / 2 and k_ccl_border takes every byte != 1 for a labelled candidate, so any
// other byte is refused here, before a launch.
int llfe_hysteresis(llfe_ctx *ctx, const uint8_t *classes, int32_t n, int32_t h, int32_t w, int32_t tile_flags,
                    uint8_t *edges, uint8_t *mask) {
    if (!ctx || !valid_dims(n, h, w) || !classes || (!edges && !mask)) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    const int cmax = chunk_for(h, w);
    if (n > cmax) return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_hysteresis: n > %d", cmax);
    const size_t P = (size_t)h * w, total = (size_t)n * P;
    const int ntx = (w + 63) >> 6, nty = (h + 63) >> 6;
    // the per-tile flag bytes in the stencil's layout: set where the tile holds a candidate
    std::vector<uint8_t> tflag(tile_flags ? (size_t)n * nty * ntx : 0, 0);
    for (size_t i = 0; i < total; i++) {
        const uint8_t b = classes[i];
        if (b > 2) return ctx->fail(LLFE_ERR_INVALID, "llfe_hysteresis: class byte %d at %zu (0, 1 or 2)", b, i);
        if (b != 1 && tile_flags) {
            const size_t img = i / P, y = (i % P) / w, x = i % w;
            tflag[img * nty * ntx + (y >> 6) * ntx + (x >> 6)] = 1;
        }
    }
    if (!n) return LLFE_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    Work &W = ctx->lanes[0].W;
    hipStream_t s = ctx->lanes[0].stream;
    HIPCHK(ctx, W.d_cls.ensure(total));
    HIPCHK(ctx, W.d_in.ensure(total));  // the 0 / 255 output of either pass
    HIPCHK(ctx, hipMemcpyAsync(W.d_cls.p, classes, total, hipMemcpyHostToDevice, s));
    if (tile_flags) {
        HIPCHK(ctx, W.d_tflag.ensure(tflag.size()));
        HIPCHK(ctx, hipMemcpyAsync(W.d_tflag.p, tflag.data(), tflag.size(), hipMemcpyHostToDevice, s));
    }
    for (int pass = 0; pass < 2; pass++) {
        uint8_t *out = pass ? mask : edges;
        if (!out) continue;
        W.tflag_valid = tile_flags != 0;  // (hyst_work takes the flags for one pass)
        HystWork wk;
        const int rc = hyst_work(ctx, W, n, h, w, &wk);
        if (rc) return rc;
        if (pass)
            HIPCHK(ctx, launch_hysteresis_dilate(W.d_cls.p, n, h, w, wk, nullptr, W.d_in.p, s));
        else
            HIPCHK(ctx, launch_canny_edges(W.d_cls.p, n, h, w, wk, W.d_in.p, s));
        HIPCHK(ctx, hipMemcpyAsync(out, W.d_in.p, total, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return LLFE_OK;
}

// dilate(src, ones(3, 3)) of the shapes path (shape pyc @L6-30) on n u8 images
int llfe_dilate3(llfe_ctx *ctx, const uint8_t *src, uint8_t *dst, int32_t n, int32_t h, int32_t w,
                 llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || !src || !dst || src == dst) return LLFE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, launch_dilate3_u8(src, n, h, w, dst, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    return LLFE_OK;
}

int llfe_shadow_stats(llfe_ctx *ctx, const uint8_t *bgr, uint64_t *sums, uint64_t *counts, int32_t n, int32_t h,
                      int32_t w, llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || !bgr || !sums || !counts) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    Work &W = ctx->lanes[0].W;
    HIPCHK(ctx, W.d_shadow.ensure(2 * (size_t)n + stencil_parts(n, h, w)));
    HIPCHK(ctx, launch_stencil(bgr, n, h, w, nullptr, nullptr, W.d_shadow.p, W.d_shadow.p + n,
                               (uint2 *)(W.d_shadow.p + 2 * n), ctx->sp, s));
    HIPCHK(ctx, hipMemcpyAsync(sums, W.d_shadow.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(counts, W.d_shadow.p + n, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return LLFE_OK;
}

int llfe_color_unique(llfe_ctx *ctx, const llfe_batch *b, uint64_t seed, uint32_t *keys, int64_t *n_unique,
                      llfe_stream stream) {
    if (!ctx || !b || !keys || !n_unique || !valid_dims(b->n, b->height, b->width)) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    const int cmax = chunk_for(b->height, b->width);
    if (b->n > cmax) return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_color_unique: n > %d", cmax);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    Work &W = ctx->lanes[0].W;
    const int h = b->height, w = b->width, n = b->n;
    const int64_t P = (int64_t)h * w;
    const int64_t key_stride = (std::max<int64_t>(P, 1) + 3) & ~int64_t(3);
    const uint8_t *img;
    const int8_t *noise;
    int rc = stage_input(ctx, W, b, 0, n, &img, &noise, s);
    if (rc) return rc;
    ImgIndex index;
    rc = chunk_index(ctx, W, b, 0, n, s, &index);
    if (rc) return rc;
    rc = color_stage(ctx, W, img, nullptr, noise, n, h, w, seed, index, /*contiguous_keys=*/true, s);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy2DAsync(keys, sizeof(uint32_t) * P, W.d_keys.p, sizeof(uint32_t) * key_stride,
                                 sizeof(uint32_t) * P, n, hipMemcpyDeviceToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(n_unique, W.d_nuniq.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return LLFE_OK;
}

int llfe_kmeans(llfe_ctx *ctx, const uint32_t *keys, int64_t key_stride, const int64_t *n_points, int32_t n,
                int32_t n_colors, uint64_t seed, int64_t index_base, llfe_image_result *results,
                llfe_stream stream) {
    if (!ctx || !keys || !n_points || !results || n < 0) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    if (key_stride % 4 || ((uintptr_t)keys & 15))
        return ctx->fail(LLFE_ERR_INVALID, "keys must be 16-byte aligned with key_stride % 4 == 0");
    if (n > kMaxKmeansBatch) return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_kmeans: n > %d", kMaxKmeansBatch);
    for (int i = 0; i < n; i++)
        if (n_points[i] < 0 || n_points[i] > key_stride) return ctx->fail(LLFE_ERR_INVALID, "n_points out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    Work &W = ctx->lanes[0].W;
    HIPCHK(ctx, W.d_nuniq.ensure(n));
    HIPCHK(ctx, hipMemcpyAsync(W.d_nuniq.p, n_points, sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
    const KmeansCubes none{nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr};  // plain sweeps over caller-supplied keys
    int rc = kmeans_stage(ctx, W, keys, key_stride, W.d_nuniq.p, n, n_colors, seed, ImgIndex{index_base, nullptr}, none, s);
    if (rc) return rc;
    HIPCHK(ctx, ctx->h_kout.ensure(n));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_kout.p, W.d_kout.p, sizeof(KmeansImageOut) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (int i = 0; i < n; i++) {
        std::memset(&results[i], 0, sizeof(llfe_image_result));
        results[i].shadow_level = -1;
        fill_color_result(ctx->h_kout.p[i], results[i]);
    }
    return LLFE_OK;
}

int llfe_palette_rules(const uint8_t *centers_rgb, const int32_t *counts, int32_t k, llfe_image_result *r) {
    if (!r || k < 0 || k > kMaxColors || (k > 0 && (!centers_rgb || !counts))) return LLFE_ERR_INVALID;
    r->n_colors = k;
    for (int i = 0; i < k; i++) {
        r->counts[i] = counts[i];
        for (int j = 0; j < 3; j++) r->centers_rgb[i][j] = centers_rgb[3 * i + j];
    }
    fill_palette(*r);
    return LLFE_OK;
}

// The attempt records of the first n images of the last k-means launch (km_last: lane 0 for the
// synchronous entry points, the ticket's lane for llfe_submit_batch / llfe_submit_images)
static int read_attempts(llfe_ctx *ctx, int32_t n, const char *who, std::vector<KmeansAttemptOut> &a,
                         int *n_colors) {
    if (ctx->any_inflight())
        return ctx->fail(LLFE_ERR_INVALID, "%s with submitted batches not yet collected", who);
    if (!ctx->km_last) return ctx->fail(LLFE_ERR_INVALID, "no k-means launch yet");
    Work &W = *ctx->km_last;
    if (n > W.km_n) return ctx->fail(LLFE_ERR_INVALID, "the last k-means launch had %d images", W.km_n);
    *n_colors = W.km_colors;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    a.resize((size_t)n * kAttempts);
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(a.data(), W.d_att.p, sizeof(KmeansAttemptOut) * a.size(), hipMemcpyDeviceToHost));
    return LLFE_OK;
}

int llfe_kmeans_attempts_k(llfe_ctx *ctx, int32_t n, int32_t k_cap, float *pp_centers, float *centers,
                           int32_t *counts, int32_t *iters, double *compactness) {
    if (!ctx || !pp_centers || !centers || !counts || !iters || !compactness || n < 0 || k_cap < 1)
        return LLFE_ERR_INVALID;
    std::vector<KmeansAttemptOut> a;
    int colors = 0;
    if (int rc = read_attempts(ctx, n, __func__, a, &colors)) return rc;
    if (colors > k_cap) return ctx->fail(LLFE_ERR_INVALID, "the last k-means launch had n_colors %d > k_cap", colors);
    const bool big = colors > kMaxK;  // k_kmeans_big keeps its k-means++ centres in a field of its own
    for (size_t i = 0; i < a.size(); i++) {
        for (int k = 0; k < k_cap; k++) {
            // an image's K = min(n_colors, U) rows: after Lloyd every cluster holds a point, and
            // the kernels write zero counts past K; K <= 1 runs no attempt (iters 0)
            const bool in = k < colors && a[i].iters > 0 && a[i].counts[k] > 0;
            for (int j = 0; j < 3; j++) {
                pp_centers[(i * k_cap + k) * 3 + j] = !in ? 0.f : big ? a[i].pp_centers_big[k][j] : a[i].pp_centers[k][j];
                centers[(i * k_cap + k) * 3 + j] = in ? a[i].centers[k][j] : 0.f;
            }
            counts[i * k_cap + k] = in ? a[i].counts[k] : 0;
        }
        iters[i] = a[i].iters;
        compactness[i] = a[i].compactness;
    }
    return LLFE_OK;
}

int llfe_kmeans_attempts(llfe_ctx *ctx, int32_t n, llfe_kmeans_attempt *out) {
    if (!ctx || !out || n < 0) return LLFE_ERR_INVALID;
    std::vector<KmeansAttemptOut> a;
    int colors = 0;
    if (int rc = read_attempts(ctx, n, __func__, a, &colors)) return rc;
    if (colors > kMaxK) return ctx->fail(LLFE_ERR_UNSUPPORTED, "attempt records only for n_colors <= %d", kMaxK);
    for (size_t i = 0; i < a.size(); i++) {
        llfe_kmeans_attempt &r = out[i];
        std::memset(&r, 0, sizeof r);
        for (int k = 0; k < kMaxK; k++) {
            for (int j = 0; j < 3; j++) {
                r.pp_centers[k][j] = a[i].pp_centers[k][j];
                r.centers[k][j] = a[i].centers[k][j];
            }
            r.counts[k] = a[i].counts[k];
        }
        r.iters = a[i].iters;
        r.compactness = a[i].compactness;
    }
    return LLFE_OK;
}

int llfe_find_contours(const uint8_t *mask, int32_t h, int32_t w, int32_t *points, int64_t points_capacity,
                       int32_t *offsets, int32_t offsets_capacity, int64_t *needed_points) {
    if (!mask || h <= 0 || w <= 0) return LLFE_ERR_INVALID;
    std::vector<int8_t> work;
    Contours c;
    external_contours_u8(mask, h, w, work, c);
    const int nc = (int)c.start.size() - 1;
    const int64_t npts = (int64_t)c.xy.size() / 2;
    if (needed_points) *needed_points = npts;
    if (npts > points_capacity || nc + 1 > offsets_capacity) return LLFE_ERR_CAPACITY;
    // output in cv2 order (newest first)
    int64_t wpos = 0;
    offsets[0] = 0;
    for (int k = 0; k < nc; k++) {
        int src = nc - 1 - k;
        int64_t a = c.start[src], b2 = c.start[src + 1];
        std::memcpy(points + 2 * wpos, c.xy.data() + 2 * a, sizeof(int32_t) * 2 * (b2 - a));
        wpos += b2 - a;
        offsets[k + 1] = (int32_t)wpos;
    }
    return nc;
}

int llfe_find_contours_gpu(llfe_ctx *ctx, const uint8_t *mask, int32_t h, int32_t w, int32_t *points,
                           int64_t points_capacity, int32_t *offsets, int32_t offsets_capacity,
                           int64_t *needed_points) {
    if (!ctx || !mask || h <= 0 || w <= 0 || !valid_dims(1, h, w)) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    int rc = gpu_contours_of_masks(ctx, mask, 1, h, w);
    if (rc) return rc;
    Work &W = ctx->lanes[0].W;
    const CtCounters ct = *ctx->slots[0].h_ct_ctr.p;
    const int *info = ctx->slots[0].h_ct_info.p;
    const int base = info[1], nc = info[2];
    std::vector<int2> refs(nc);
    std::vector<CtComp> comps(ct.comps);
    std::vector<int2> pts(ct.pts);
    if (nc) HIPCHK(ctx, hipMemcpy(refs.data(), W.d_ct_refs.p + base, sizeof(int2) * nc, hipMemcpyDeviceToHost));
    if (ct.comps) HIPCHK(ctx, hipMemcpy(comps.data(), W.d_ct_comps.p, sizeof(CtComp) * ct.comps, hipMemcpyDeviceToHost));
    if (ct.pts) HIPCHK(ctx, hipMemcpy(pts.data(), W.d_ct_pts.p, sizeof(int2) * ct.pts, hipMemcpyDeviceToHost));
    int64_t npts = 0;
    for (int k = 0; k < nc; k++) npts += comps[refs[k].x].nv;
    if (needed_points) *needed_points = npts;
    if (npts > points_capacity || nc + 1 > offsets_capacity) return LLFE_ERR_CAPACITY;
    int64_t wpos = 0;  // cv2 order: newest first
    offsets[0] = 0;
    for (int k = 0; k < nc; k++) {
        const CtComp &c = comps[refs[nc - 1 - k].x];
        for (uint32_t v = 0; v < c.nv; v++) {
            points[2 * (wpos + v)] = pts[c.off + v].x;
            points[2 * (wpos + v) + 1] = pts[c.off + v].y;
        }
        wpos += c.nv;
        offsets[k + 1] = (int32_t)wpos;
    }
    return nc;
}

int llfe_shapes_from_masks_gpu(llfe_ctx *ctx, const uint8_t *masks, int32_t n, int32_t h, int32_t w,
                               llfe_shape *shapes, int64_t capacity, int32_t *n_shapes, int32_t *n_contours,
                               int64_t *needed) {
    if (!ctx || !masks || !valid_dims(n, h, w) || n <= 0) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    int rc = gpu_contours_of_masks(ctx, masks, n, h, w);
    if (rc) return rc;
    const int *info = ctx->slots[0].h_ct_info.p;
    const llfe_shape *src = ctx->slots[0].h_ct_shapes.p;
    int64_t total = 0;
    for (int i = 0; i < n; i++) {
        const int nk = info[i * kCtInfo + 3], sb = info[i * kCtInfo + 4];
        if (n_shapes) n_shapes[i] = nk;
        if (n_contours) n_contours[i] = info[i * kCtInfo + 2];
        for (int k = 0; k < nk; k++)
            if (shapes && total + k < capacity) shapes[total + k] = src[sb + k];
        total += nk;
    }
    if (needed) *needed = total;
    return total > capacity ? LLFE_ERR_CAPACITY : LLFE_OK;
}

// FontDetector.detect_font after its binary (font_detector.py:39-67, :109-155) on lane 0's
// workspace and the caller's stream: binary -> bit rows -> boxes-only contour pass -> region
// filter, largest region, its gray sum (font.hip).  One D2H of the records per device pass,
// and of the region list when it is asked for.
int llfe_font_detect(llfe_ctx *ctx, const uint8_t *bgr, const uint8_t *binary, int32_t n, int32_t h, int32_t w,
                     llfe_font_result *results, int32_t *regions, int64_t region_capacity, int64_t *regions_needed,
                     llfe_stream stream) {
    if (!ctx || !valid_dims(n, h, w) || (!bgr && !binary) || !results || (regions && region_capacity < 0))
        return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    if (w > kCtMaxWidth || h > kCtMaxHeight)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_font_detect needs width <= %d and height <= %d", kCtMaxWidth,
                         kCtMaxHeight);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    Work &W = ctx->lanes[0].W;
    HostBuf<CtCounters> &h_ctr = ctx->slots[0].h_ct_ctr;
    const int chunk = chunk_for(h, w);
    const size_t P = (size_t)h * w;
    int64_t total = 0;
    HIPCHK(ctx, h_ctr.ensure(1));
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const uint8_t *img = bgr ? bgr + (size_t)i0 * P * 3 : nullptr;
        const uint8_t *bin = binary ? binary + (size_t)i0 * P : nullptr;
        if (!bin) {
            HIPCHK(ctx, W.d_cls.ensure((size_t)m * P));
            W.tflag_valid = false;  // d_cls no longer holds a class map
            TIMED(ctx, s, "k_font_binary", (double)m * P * 4, launch_font_binary(img, m, h, w, W.d_cls.p, ctx->sp, s));
            bin = W.d_cls.p;
        }
        HIPCHK(ctx, W.d_bits.ensure((size_t)m * h * words_per_row(w)));
        TIMED(ctx, s, "k_font_pack", (double)m * P * (1 + 0.125), launch_font_pack(bin, m, h, w, W.d_bits.p, s));
        HIPCHK(ctx, W.d_font_rec.ensure((size_t)m));
        for (int attempt = 0;; attempt++) {
            const int rc = run_contours(ctx, W, m, h, w, W.d_bits.p, s, true);
            if (rc) return rc;
            TIMED(ctx, s, "k_font_select", 0.0,
                  launch_font_select(W.d_ct_comps.p, W.d_ct_refs.p, W.d_ct_info.p, m, W.d_font_rec.p, s));
            if (img) TIMED(ctx, s, "k_font_gray_sum", 0.0, launch_font_gray_sum(img, m, h, w, W.d_font_rec.p, s));
            HIPCHK(ctx, hipMemcpyAsync(h_ctr.p, W.d_ct_ctr.p, sizeof(CtCounters), hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipMemcpyAsync(results + i0, W.d_font_rec.p, sizeof(llfe_font_result) * m,
                                       hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
            const CtCounters ct = *h_ctr.p;
            if (ct.flags & ~kCtOverflowMask)
                return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_font_detect: unsupported mask (flags 0x%x)", ct.flags);
            if (!(ct.flags & kCtOverflowMask)) break;
            if (attempt >= 8) return ctx->fail(LLFE_ERR_CAPACITY, "llfe_font_detect: capacities still overflow");
            grow_contour_caps(W, m, h, w, ct);
        }
        int64_t chunk_total = 0;
        for (int i = 0; i < m; i++) {
            results[i0 + i].region_offset = total + chunk_total;
            chunk_total += results[i0 + i].n_regions;
        }
        const int64_t room = std::max<int64_t>(0, std::min(chunk_total, region_capacity - total));
        if (regions && room > 0) {
            HIPCHK(ctx, W.d_font_reg.ensure((size_t)room));
            TIMED(ctx, s, "k_font_regions", 0.0,
                  launch_font_regions(W.d_ct_comps.p, W.d_ct_refs.p, W.d_ct_info.p, m, W.d_font_rec.p, W.d_font_reg.p,
                                      room, s));
            HIPCHK(ctx, hipMemcpyAsync(regions + 4 * total, W.d_font_reg.p, sizeof(int4) * (size_t)room,
                                       hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
        }
        total += chunk_total;
    }
    ctx->prof.collect(-2);
    if (regions_needed) *regions_needed = total;
    if (regions && total > region_capacity)
        return ctx->fail(LLFE_ERR_CAPACITY, "region capacity %lld < %lld", (long long)region_capacity, (long long)total);
    return LLFE_OK;
}

double llfe_border_radius(const int32_t *points, int32_t n, double epsilon_factor) {
    if (!points || n <= 0) return 0.0;
    ShapeScratch sc;
    return border_radius(points, n, epsilon_factor, sc);
}

int llfe_classify_contour(const int32_t *points, int32_t n, llfe_shape *out) {
    if (!points || n <= 0 || !out) return n == 0 ? 0 : LLFE_ERR_INVALID;
    ShapeScratch sc;
    return classify_contour(points, n, sc, *out) ? 1 : 0;
}

int llfe_shapes_from_mask(const uint8_t *mask, int32_t h, int32_t w, llfe_shape *shapes, int32_t capacity,
                          int32_t *n_contours) {
    if (!mask || h <= 0 || w <= 0) return LLFE_ERR_INVALID;
    std::vector<int8_t> work;
    Contours c;
    ShapeScratch sc;
    std::vector<llfe_shape> out;
    external_contours_u8(mask, h, w, work, c);
    int nc = shapes_from_contours(c, sc, out);
    if (n_contours) *n_contours = nc;
    if ((int64_t)out.size() > capacity) return LLFE_ERR_CAPACITY;
    for (size_t i = 0; i < out.size(); i++) shapes[i] = out[i];
    return (int)out.size();
}

}  // extern "C"
