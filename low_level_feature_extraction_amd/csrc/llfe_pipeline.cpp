// C ABI of libllfe.so (include/llfe.h): the batch pipeline that replaces the native work
// behind ColorExtractor.extract_colors, ShapeAnalyzer.analyze_shapes,
// ShadowAnalyzer.analyze_shadow_level and FontDetector.detect_font, and the stage helpers
// it shares with the stage drop-ins (llfe_stages.cpp).
//
// Per chunk of images (all on the caller's stream):
//   stencil (gray/blur5/Canny-NMS/adaptive mean)  -> class map + shadow sums
//   hysteresis as connected components (4 launches) fused with dilate + bit-pack
//   -> D2H (1 bit / pixel)
//   colour bitmap -> compaction -> k-means (10 attempts / image) -> D2H 64 B / image
//   host thread pool: external contours + shape geometry from the packed masks
#include <chrono>
#include <map>

#include "llfe_ctx.h"

using namespace llfe_host;

namespace llfe_host {

// The stage entry points run on lane 0, host slot 0's buffers and the caller's stream:
// refused while submitted batches (one of which may own lane 0) are not collected.  Their
// profiler records carry the stage tag, so llfe_collect_batch never takes them for a
// slot's.
int stage_enter(llfe_ctx *ctx, const char *fn) {
    if (ctx->any_inflight())
        return ctx->fail(LLFE_ERR_INVALID, "%s with submitted batches not yet collected", fn);
    ctx->prof.cur_slot = Profiler::kStageSlot;
    return LLFE_OK;
}

int stage_input(llfe_ctx *ctx, Work &W, const llfe_batch *b, int i0, int n, const uint8_t **d_img, const int8_t **d_noise,
                hipStream_t s) {
    size_t P3 = (size_t)b->height * b->width * 3;
    const bool h2d = !b->on_device || (b->noise && !b->noise_on_device);
    if (h2d && ctx->h2d_pending) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->h2d_done, 0));
    if (b->on_device) {
        *d_img = b->data + (size_t)i0 * P3;
    } else {
        HIPCHK(ctx, W.d_in.ensure(P3 * n));
        HIPCHK(ctx, hipMemcpyAsync(W.d_in.p, b->data + (size_t)i0 * P3, P3 * n, hipMemcpyHostToDevice, s));
        *d_img = W.d_in.p;
    }
    *d_noise = nullptr;
    if (b->noise) {
        if (b->noise_on_device) {
            *d_noise = b->noise + (size_t)i0 * P3;
        } else {
            HIPCHK(ctx, W.d_noise.ensure(P3 * n));
            HIPCHK(ctx, hipMemcpyAsync(W.d_noise.p, b->noise + (size_t)i0 * P3, P3 * n, hipMemcpyHostToDevice, s));
            *d_noise = W.d_noise.p;
        }
    }
    if (h2d) {
        HIPCHK(ctx, hipEventRecord(ctx->h2d_done, s));
        ctx->h2d_pending = true;
    }
    return LLFE_OK;
}

// The hysteresis workspace of an n x h x w batch, grown on demand.
int hyst_work(llfe_ctx *ctx, Work &W, int n, int h, int w, HystWork *out) {
    const size_t ids = hysteresis_ids(n, h, w);
    const size_t tiles = (size_t)tiles_x(w) * tiles_y(h) * n;
    HIPCHK(ctx, W.d_lab.ensure((size_t)n * h * w));
    HIPCHK(ctx, W.d_parent.ensure(ids));
    HIPCHK(ctx, W.d_sroot.ensure(ids));
    HIPCHK(ctx, W.d_roots.ensure(ids));
    HIPCHK(ctx, W.d_nroots.ensure(tiles));
    HIPCHK(ctx, W.d_tstrong.ensure(hysteresis_tiles(n, h, w) * hysteresis_tile_words()));
    HIPCHK(ctx, W.d_ebits.ensure((size_t)n * h * words_per_row(w)));
    HIPCHK(ctx, W.d_ftlist.ensure(tiles + 2));
    HIPCHK(ctx, W.d_ptlist.ensure(tiles + 1));
    *out = HystWork{W.d_lab.p,     W.d_parent.p, W.d_sroot.p,       W.d_roots.p,   W.d_nroots.p,
                    W.d_tstrong.p, W.d_ebits.p,
                    W.tflag_valid ? W.d_tflag.p : nullptr, W.d_ftlist.p + 2, W.d_ftlist.p,
                    W.d_ptlist.p};
    W.tflag_valid = false;  // (one hysteresis pass per stencil launch)
    return LLFE_OK;
}

// The stencil parameters of a class-map launch into W.d_cls: the hysteresis tile flags
// (zeroed here, on s) that let the hysteresis skip the tiles without a Canny candidate.
int stencil_params(llfe_ctx *ctx, Work &W, int n, int h, int w, hipStream_t s, StencilParams *sp) {
    *sp = ctx->sp;
    W.tflag_valid = false;
    // LLFE_HYST_TILE_FLAGS=0: no flags, the hysteresis visits every tile (its test path)
    if (const char *e = getenv("LLFE_HYST_TILE_FLAGS"))
        if (!strcmp(e, "0")) return LLFE_OK;
    const size_t tiles = (size_t)n * tiles_x(w) * ((h + 63) / 64);
    HIPCHK(ctx, W.d_tflag.ensure(tiles));
    HIPCHK(ctx, hipMemsetAsync(W.d_tflag.p, 0, tiles, s));
    sp->tflag = W.d_tflag.p;
    W.tflag_valid = true;
    return LLFE_OK;
}

// Canny hysteresis (connected components) + dilate + pack of W.d_cls.
int run_hysteresis_dilate(llfe_ctx *ctx, Work &W, int n, int h, int w, uint64_t *bits, uint8_t *mask_u8, hipStream_t s) {
    HystWork wk;
    const int rc = hyst_work(ctx, W, n, h, w, &wk);
    if (rc) return rc;
    // algorithmic bytes (which folds hysteresis into the fused 4P stencil
    // front): what any implementation of this stage must move -- the class map read (P) and
    // the bit-packed dilated mask written (P/8).  The CC labels and tile bitmaps it also
    // reads and writes are the implementation's (PMC saw ~2.4 P per image, round 4).
    TIMED(ctx, s, "k_hysteresis_dilate", (double)n * h * w * (1 + 0.125),
          launch_hysteresis_dilate(W.d_cls.p, n, h, w, wk, bits, mask_u8, s));
    return LLFE_OK;
}

// External contours + shape records of W.d_bits on the GPU (hysteresis workspace reused);
// boxes: the boxes-only mode (no vertex, staging or shape storage)
int run_contours(llfe_ctx *ctx, Work &W, int n, int h, int w, const uint64_t *bits, hipStream_t s, bool boxes) {
    CtCaps c = contours_default_caps(n, h, w);
    c.comps = std::max(c.comps, W.ct_min.comps);
    c.pts = std::max(c.pts, W.ct_min.pts);
    c.refs = std::max(c.refs, W.ct_min.refs);
    c.shapes = std::max(c.shapes, W.ct_min.shapes);
    const size_t ids = hysteresis_ids(n, h, w);
    HIPCHK(ctx, W.d_lab.ensure((size_t)n * h * w));
    HIPCHK(ctx, W.d_parent.ensure(ids));
    HIPCHK(ctx, W.d_roots.ensure(ids));
    HIPCHK(ctx, W.d_nroots.ensure((size_t)tiles_x(w) * tiles_y(h) * n));
    HIPCHK(ctx, W.d_ct_planes.ensure(5 * contours_plane_words(n, h, w)));
    HIPCHK(ctx, W.d_ct_comps.ensure(c.comps));
    HIPCHK(ctx, W.d_ct_acc.ensure(c.comps));
    if (!boxes) HIPCHK(ctx, W.d_ct_pts.ensure(c.pts));
    HIPCHK(ctx, W.d_ct_refs.ensure(c.refs));
    if (!boxes) HIPCHK(ctx, W.d_ct_stage.ensure((size_t)kCtTraceBlocks * kCtStage));
    HIPCHK(ctx, W.d_ct_ctr.ensure(1));
    HIPCHK(ctx, W.d_ct_info.ensure((size_t)n * kCtInfo));
    if (!boxes) HIPCHK(ctx, W.d_ct_shapes.ensure(c.shapes));
    CtWork wk{W.d_lab.p, W.d_parent.p, W.d_roots.p, W.d_nroots.p, W.d_ct_planes.p, W.d_ct_comps.p, W.d_ct_acc.p,
              W.d_ct_pts.p, W.d_ct_refs.p, W.d_ct_stage.p, W.d_ct_ctr.p, W.d_ct_info.p, W.d_ct_shapes.p, c};
    // algorithmic bytes: mask bits read by components + scan, labels written and read
    if (boxes)
        TIMED(ctx, s, "k_contours_boxes", (double)n * h * w * (0.25 + 4.0), launch_contours(bits, n, h, w, wk, s, true));
    else
        TIMED(ctx, s, "k_contours", (double)n * h * w * (0.25 + 4.0), launch_contours(bits, n, h, w, wk, s));
    return LLFE_OK;
}

// enqueue the D2H of a contour pass's results into host slot H on stream cs
int copy_contours(llfe_ctx *ctx, Work &W, int n, HostSlot &H, hipStream_t cs) {
    HIPCHK(ctx, H.h_ct_info.ensure((size_t)n * kCtInfo));
    HIPCHK(ctx, H.h_ct_ctr.ensure(1));
    HIPCHK(ctx, H.h_ct_shapes.ensure(W.d_ct_shapes.n));
    H.ct_shape_cap = (int64_t)W.d_ct_shapes.n;
    HIPCHK(ctx, hipMemcpyAsync(H.h_ct_info.p, W.d_ct_info.p, sizeof(int) * n * kCtInfo, hipMemcpyDeviceToHost, cs));
    HIPCHK(ctx, hipMemcpyAsync(H.h_ct_ctr.p, W.d_ct_ctr.p, sizeof(CtCounters), hipMemcpyDeviceToHost, cs));
    HIPCHK(ctx, hipMemcpyAsync(H.h_ct_shapes.p, W.d_ct_shapes.p, sizeof(llfe_shape) * W.d_ct_shapes.n,
                               hipMemcpyDeviceToHost, cs));
    return LLFE_OK;
}

// grow the contour capacities after an overflowing pass (counters hold what was asked)
void grow_contour_caps(Work &W, int n, int h, int w, const CtCounters &ct) {
    const CtCaps d = contours_default_caps(n, h, w);
    CtCaps &m = W.ct_min;
    auto up = [](int64_t cur, int64_t dflt, int64_t need) { return std::max({2 * std::max(cur, dflt), need + need / 4}); };
    if (ct.flags & kCtOverflowComps) m.comps = up(m.comps, d.comps, (int64_t)ct.comps + (int64_t)n * kCtQuirkCap);
    if (ct.flags & kCtOverflowPts) m.pts = up(m.pts, d.pts, (int64_t)ct.pts);
    if (ct.flags & (kCtOverflowRefs | kCtOverflowComps))
        m.refs = up(m.refs, d.refs, std::max<int64_t>(m.comps, d.comps) + (int64_t)n * kCtQuirkCap);
    if (ct.flags & kCtOverflowShapes) m.shapes = up(m.shapes, d.shapes, (int64_t)ct.shapes);
}

// contiguous_keys: also gather each image's unique keys into W.d_keys in np.unique order
// (llfe_color_unique's output, the general-K k-means); otherwise they stay where k_uq_part
// wrote them (W.d_raw, partition R at the prefix of the partition pixel counts) and the cube
// k-means reads them there (KmeansCubes::part_hist)
// ragged (a pass of images of any sizes): h x w is its largest image, which sizes every
// stride, the run table rows and the noise field; `noise` non-null says that the records
// carry parity noise
int color_stage(llfe_ctx *ctx, Work &W, const uint8_t *img, const uint64_t *img_tab, const int8_t *noise, int n, int h,
                int w, uint64_t seed, ImgIndex index, bool contiguous_keys, hipStream_t s, const UqImages *ragged) {
    // unique colours -> W.d_keys (sorted, key_stride) + cube table for k-means
    const int64_t P = (int64_t)h * w;
    const int64_t key_stride = (std::max<int64_t>(P, 1) + 3) & ~int64_t(3);
    const int64_t cube_stride = std::min<int64_t>(key_stride, kMaxCubes);
    const int64_t cell_stride = std::min<int64_t>(cube_stride, (int64_t)kParts * kCellsPerPart);
    HIPCHK(ctx, W.d_raw.ensure((size_t)n * key_stride));
    HIPCHK(ctx, W.d_keys.ensure((size_t)n * key_stride));
    HIPCHK(ctx, W.d_segcubes.ensure((size_t)n * kParts * kCubesPerPart));
    HIPCHK(ctx, W.d_cubes.ensure((size_t)n * cube_stride));
    HIPCHK(ctx, W.d_segcells.ensure((size_t)n * kParts * kCellsPerPart));
    HIPCHK(ctx, W.d_cells.ensure((size_t)n * cell_stride));
    HIPCHK(ctx, W.d_ncells.ensure(n));
    HIPCHK(ctx, W.d_sups.ensure((size_t)n * cell_stride));
    HIPCHK(ctx, W.d_nsups.ensure(n));
    HIPCHK(ctx, W.d_pmeta.ensure((size_t)n * kParts * 5));
    HIPCHK(ctx, W.d_nuniq.ensure(n));
    HIPCHK(ctx, W.d_ncubes.ensure(n));
    HIPCHK(ctx, W.d_pmom.ensure((size_t)n * kPartMoments * kParts));
    // (d_pmeta: hist, cl, uq, cc, cs; k-means reads uq)
    uint32_t *hist = W.d_pmeta.p, *cl = hist + (size_t)n * kParts, *uq = hist + (size_t)2 * n * kParts,
             *cc = uq + (size_t)n * kParts, *cs = cc + (size_t)n * kParts;
    HIPCHK(ctx, hipMemsetAsync(hist, 0, sizeof(uint32_t) * n * kParts, s));
    HIPCHK(ctx, W.d_segtab.ensure((size_t)n * uq_tab_words(P)));
    if (!noise) {
        HIPCHK(ctx, W.d_nfield.ensure((size_t)noise_field_pixels(P)));
        HIPCHK(ctx, launch_uq_noise(noise, W.d_nfield.p, P, seed, s));
    }
    // Algorithmic bytes (colour pass 3P + 4 MiB + 8U per image): the scatter
    // is charged the input read (3P, + 3P of parity noise when given), k_uq_part the 2^24-bit
    // presence bitmap's clear + scan (4 MiB; held in LDS here) and the unique-key write (4U),
    // k_uq_gather the key read (4U); the step segments written and read back between the
    // scatter and k_uq_part (4P each way) are the implementation's, not counted.
    // keys -> per-step segments sorted by partition + run table + partition totals
    TIMED(ctx, s, "k_uq_scatter", (double)(ragged ? ragged->pixels : n * P) * (noise ? 6 : 3),
          launch_uq_scatter(img, img_tab, noise, W.d_nfield.p, n, h, w, seed, index, key_stride, hist, W.d_segtab.p,
                            W.d_keys.p, s, ragged));
    // the partitions' sorted unique keys go to the (free) d_raw
    TIMED(ctx, s, "k_uq_part", (double)n * 4194304.0,
          launch_uq_part(W.d_keys.p, n, key_stride, P, hist, W.d_segtab.p, W.d_raw.p, W.d_segcubes.p,
                         W.d_segcells.p, uq, cc, cl, cs, s, ragged));
    TIMED(ctx, s, "k_uq_gather", 0,
          launch_uq_gather(W.d_raw.p, n, key_stride, hist, uq, cc, cl, cs, W.d_segcubes.p, W.d_segcells.p,
                           W.d_keys.p, W.d_cubes.p, W.d_cells.p, W.d_sups.p, cube_stride, cell_stride,
                           cell_stride, W.d_nuniq.p, W.d_ncubes.p, W.d_ncells.p, W.d_nsups.p, W.d_pmom.p,
                           contiguous_keys, s));
    return LLFE_OK;
}

int kmeans_stage(llfe_ctx *ctx, Work &W, const uint32_t *keys, int64_t key_stride, const int64_t *d_nuniq, int n,
                 int n_colors, uint64_t seed, ImgIndex index, const KmeansCubes &cubes, hipStream_t s) {
    if (n_colors < 1 || n_colors > kMaxColors)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "n_colors must be in [1, LLFE_MAX_COLORS]");
    const int64_t sstride = kmeans_scratch_stride(key_stride);
    HIPCHK(ctx, W.d_order.ensure((size_t)n + 2));  // LPT order + the two work-queue counters
    HIPCHK(ctx, W.d_kscratch.ensure((size_t)n * kAttempts * sstride));
    HIPCHK(ctx, W.d_att.ensure((size_t)n * kAttempts));
    HIPCHK(ctx, W.d_kout.ensure(n));
    W.km_n = n;
    W.km_colors = n_colors;
    ctx->km_last = &W;
    // per-image cv::RNG state = splitmix64(seed + global index) is derived on the device
    TIMED(ctx, s, "k_kmeans", 0,
          launch_kmeans(keys, key_stride, d_nuniq, n, n_colors, seed, index, W.d_order.p, W.d_kscratch.p,
                        sstride, W.d_att.p, W.d_kout.p, cubes, s));
    if (const char *path = getenv("LLFE_KM_TRACE")) {  // debug: per-attempt timeline + U
        std::vector<KmeansAttemptOut> att((size_t)n * kAttempts);
        std::vector<int64_t> nu(n);
        HIPCHK(ctx, hipMemcpyAsync(att.data(), W.d_att.p, sizeof(KmeansAttemptOut) * att.size(),
                                   hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(nu.data(), d_nuniq, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        if (FILE *f = fopen(path, "a")) {
            for (int i = 0; i < n; i++)
                for (int a = 0; a < kAttempts; a++) {
                    const KmeansAttemptOut &o = att[(size_t)i * kAttempts + a];
                    fprintf(f, "%d %d %lld %d %llu %llu %u %u %llu %llu %llu %u %u %d %llu %llu %llu %llu %llu %llu %llu %u %u %u %u %u %u %u %u %u\n", i, a, (long long)nu[i], o.iters,
                            (unsigned long long)o.t_start, (unsigned long long)o.t_end, o.hw_id, o.xcc_id,
                            (unsigned long long)o.t_pp, (unsigned long long)o.t_lloyd, (unsigned long long)o.bytes, o.pp_pts, o.n_cubes, o.pad, (unsigned long long)o.t_sel,
                            (unsigned long long)o.ll_pts, (unsigned long long)o.t_sw, (unsigned long long)o.split_cubes,
                            (unsigned long long)o.split_pts, (unsigned long long)o.drift_hist,
                            (unsigned long long)o.t_lstart, o.hw_id2, o.xcc_id2, o.pp_split_cubes, o.pp_split_pts,
                            o.split_walks, o.split_partial, o.pp_walks, o.pp_walk_lanes, o.pp_walk_mixed);
                }
            fclose(f);
        }
    }
    return LLFE_OK;
}

// ColorExtractor.is_light_color (color_extractor.py:67-71), in the reference's order
static bool is_light_color(int r, int g, int b) {
    const double R = r / 255.0, G = g / 255.0, B = b / 255.0;
    return 0.2126 * R + 0.7152 * G + 0.0722 * B > 0.6;
}

// extract_colors' palette rules (color_extractor.py:231-284) on r's centres and counts:
// frequency order (stable on ties; np.argsort(-counts)'s tie order is host-dependent in the
// reference), hex, '#ffffff' / '#000000' dropped, primary, three accents
// (padded with the last, or the primary), background by the primary's luminance
void fill_palette(llfe_image_result &r) {
    const int K = r.n_colors;
    int ord[kMaxColors];
    for (int i = 0; i < K; i++) ord[i] = i;
    if (K > 1) std::stable_sort(ord, ord + K, [&](int a, int b) { return r.counts[a] > r.counts[b]; });
    char hex[kMaxColors][8];
    int rgb[kMaxColors][3];
    int nh = 0;
    for (int i = 0; i < K; i++) {
        const uint8_t *c = r.centers_rgb[ord[i]];
        if ((c[0] == 255 && c[1] == 255 && c[2] == 255) || (c[0] == 0 && c[1] == 0 && c[2] == 0)) continue;
        std::snprintf(hex[nh], 8, "#%02x%02x%02x", c[0], c[1], c[2]);
        rgb[nh][0] = c[0], rgb[nh][1] = c[1], rgb[nh][2] = c[2];
        nh++;
    }
    if (nh == 0) {  // nothing left: the contrasting colour for white (:245-256)
        const char *bg = is_light_color(255, 255, 255) ? "#000000" : "#FFFFFF";
        std::snprintf(r.primary, 8, "%s", bg);
        std::snprintf(r.background, 8, "%s", bg);
        for (auto &a : r.accent) std::snprintf(a, 8, "%s", bg);
        return;
    }
    std::snprintf(r.primary, 8, "%s", hex[0]);
    int na = 0;
    for (int i = 1; i < nh && na < 3; i++)
        if (std::strcmp(hex[i], hex[0]) != 0) std::snprintf(r.accent[na++], 8, "%s", hex[i]);
    for (; na < 3; na++) std::snprintf(r.accent[na], 8, "%s", na ? r.accent[na - 1] : r.primary);
    std::snprintf(r.background, 8, "%s", is_light_color(rgb[0][0], rgb[0][1], rgb[0][2]) ? "#000000" : "#FFFFFF");
}

void fill_color_result(const KmeansImageOut &k, llfe_image_result &r) {
    r.n_colors = k.k;
    for (int c = 0; c < kMaxColors; c++) {
        r.counts[c] = k.counts[c];
        for (int j = 0; j < 3; j++) r.centers_rgb[c][j] = k.centers_rgb[c][j];
    }
    r.n_unique = k.n_unique;
    r.compactness = k.compactness;
    fill_palette(r);
}

// global indices of images [i0, i0 + n) of a batch: index_base + i, or the caller's list
// (uploaded on stream s into the workspace)
int chunk_index(llfe_ctx *ctx, Work &W, const llfe_batch *b, int i0, int n, hipStream_t s, ImgIndex *out) {
    *out = ImgIndex{b->index_base + i0, nullptr};
    if (b->indices && n > 0) {
        HIPCHK(ctx, W.d_index.ensure((size_t)n));
        HIPCHK(ctx, hipMemcpyAsync(W.d_index.p, b->indices + i0, sizeof(long long) * n, hipMemcpyHostToDevice, s));
        out->idx = W.d_index.p;
    }
    return LLFE_OK;
}

}  // namespace llfe_host

// ShadowAnalyzer.analyze_shadow_level's decision (shadow pyc @L22-31): 0 Low, 1 Moderate, 2 High
int32_t llfe_host::shadow_level(uint64_t sum, uint64_t count) {
    if (count == 0) return 0;
    const double avg_darkness = 255.0 - (double)sum / (double)count;
    return avg_darkness < 30 ? 0 : (avg_darkness < 60 ? 1 : 2);
}

namespace {

// LLFE_FEATURE_FONTS after k_font_bits, on stream s: the boxes-only contour pass over
// W.d_fbits, the region filter and largest region, its gray sum, then the D2H of the n
// records and of the pass's counters into host slot H (on s itself, so whatever follows on
// s may reuse the contour workspace).
int font_pass(llfe_ctx *ctx, Work &W, const uint8_t *img, const uint64_t *img_tab, int n, int h, int w, HostSlot &H,
              hipStream_t s) {
    HIPCHK(ctx, W.d_font_rec.ensure((size_t)n));
    HIPCHK(ctx, H.h_font_rec.ensure((size_t)n));
    HIPCHK(ctx, H.h_font_ctr.ensure(1));
    const int rc = run_contours(ctx, W, n, h, w, W.d_fbits.p, s, true);
    if (rc) return rc;
    TIMED(ctx, s, "k_font_select", 0.0,
          launch_font_select(W.d_ct_comps.p, W.d_ct_refs.p, W.d_ct_info.p, n, W.d_font_rec.p, s));
    TIMED(ctx, s, "k_font_gray_sum", 0.0, launch_font_gray_sum(img, n, h, w, W.d_font_rec.p, s, img_tab));
    HIPCHK(ctx, hipMemcpyAsync(H.h_font_ctr.p, W.d_ct_ctr.p, sizeof(CtCounters), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(H.h_font_rec.p, W.d_font_rec.p, sizeof(llfe_font_result) * n, hipMemcpyDeviceToHost, s));
    return LLFE_OK;
}

// Device half of one chunk, on lane L's streams and workspace: every kernel, then the D2H
// of the per-image results into host slot H (number `slot`: the profiler tag), with events
// the host half waits on.
// img_tab (device, llfe_submit_images): image i of the chunk at img_tab[i], read in place by
// the scatter and the stencil (b->data then only names the first image)
int enqueue_chunk(llfe_ctx *ctx, const llfe_batch *b, uint32_t features, uint64_t seed, int i0, int n, Lane &L,
                  HostSlot &H, int slot, const uint64_t *img_tab = nullptr) {
    ctx->prof.cur_slot = slot;
    Work &W = L.W;
    hipStream_t s = L.stream;
    const int h = b->height, w = b->width, wpr = words_per_row(w);
    const bool want_col = features & LLFE_FEATURE_COLORS, want_shp = features & LLFE_FEATURE_SHAPES,
               want_shd = features & LLFE_FEATURE_SHADOWS, want_fnt = features & LLFE_FEATURE_FONTS;
    const int64_t P = (int64_t)h * w;
    const int64_t key_stride = (std::max<int64_t>(P, 1) + 3) & ~int64_t(3);
    const int n_colors = b->n_colors ? b->n_colors : kMaxK;
    const uint8_t *img;
    const int8_t *noise;
    int rc = stage_input(ctx, W, b, i0, n, &img, &noise, s);
    if (rc) return rc;
    ImgIndex index;
    rc = chunk_index(ctx, W, b, i0, n, s, &index);
    if (rc) return rc;
    // the colour path (unique colours + k-means) runs on the second stream, concurrently
    // with shapes / shadows (both only read the input).  Measured (512 x 1080p): shapes
    // alongside the colour front 13.1k images/s; shapes held back to share the GPU with
    // k-means 12.8k -- the stencil waves slow the k-means attempts more than they fill
    // its tail.
    hipStream_t col_s = s;
    if (want_col && ctx->concurrent && (want_shp || want_shd || want_fnt)) {
        col_s = L.col_stream;
        HIPCHK(ctx, hipEventRecord(ctx->input_ready, s));
        HIPCHK(ctx, hipStreamWaitEvent(col_s, ctx->input_ready, 0));
    }
    // colour front (unique colours), then shapes / shadows (on the other stream), then
    // k-means
    if (want_col) {
        rc = color_stage(ctx, W, img, img_tab, noise, n, h, w, seed, index, /*contiguous_keys=*/n_colors > kMaxK, col_s);
        if (rc) return rc;
    }
    // d_shadow / d_bits of this workspace may still be in the previous chunk's D2H
    if (L.mask_reader) HIPCHK(ctx, hipStreamWaitEvent(s, L.mask_reader->mask_done, 0));
    // fonts first on this stream: the pass shares the hysteresis / contour workspace with the
    // shapes pass below, and its records and counters have left it (d_font_rec, the host
    // slot) before the shapes pass overwrites it
    H.img_tab = img_tab;
    if (want_fnt) {
        HIPCHK(ctx, W.d_fbits.ensure((size_t)n * h * wpr));
        TIMED(ctx, s, "k_font_bits", (double)n * P * (3 + 0.125), launch_font_bits(img, img_tab, n, h, w, W.d_fbits.p, s));
        // (wider / taller than the GPU contour pass takes: finish_chunk runs the host path)
        H.font_gpu = w <= kCtMaxWidth && h <= kCtMaxHeight;
        if (H.font_gpu) {
            rc = font_pass(ctx, W, img, img_tab, n, h, w, H, s);
            if (rc) return rc;
        }
    }
    if (want_shp || want_shd) {
        HIPCHK(ctx, W.d_shadow.ensure(2 * (size_t)n + stencil_parts(n, h, w)));
        StencilParams sp = ctx->sp;
        if (want_shp) {
            HIPCHK(ctx, W.d_cls.ensure((size_t)n * P));
            rc = stencil_params(ctx, W, n, h, w, s, &sp);  // (starts from ctx->sp)
            if (rc) return rc;
        }
        // after stencil_params: the stencil reads an in-place batch through its table (with
        // the packed-batch addressing, image i >= 1 would lie past image 0's allocation)
        sp.img_tab = img_tab;
        TIMED(ctx, s, "k_stencil", (double)n * P * (3 + (want_shp ? 1 : 0)),
              launch_stencil(img, n, h, w, want_shp ? W.d_cls.p : nullptr, nullptr,
                             want_shd ? W.d_shadow.p : nullptr, want_shd ? W.d_shadow.p + n : nullptr,
                             (uint2 *)(W.d_shadow.p + 2 * n), sp, s));
    }
    // shapes + shadows go to the host (event mask_done) while the GPU is still in this
    // chunk's colour stage, so contour tracing overlaps k-means
    const bool gpu_ct = ctx->gpu_contours && w <= kCtMaxWidth && h <= kCtMaxHeight;
    H.gpu_ct = gpu_ct;
    if (want_shp) {
        HIPCHK(ctx, W.d_bits.ensure((size_t)n * h * wpr));
        if (!gpu_ct) HIPCHK(ctx, H.h_bits.ensure((size_t)n * h * wpr));
        rc = run_hysteresis_dilate(ctx, W, n, h, w, W.d_bits.p, nullptr, s);
        if (rc) return rc;
        if (gpu_ct) {
            rc = run_contours(ctx, W, n, h, w, W.d_bits.p, s);
            if (rc) return rc;
        }
    }
    if (want_shd) HIPCHK(ctx, H.h_shadow.ensure(2 * (size_t)n));
    if (want_shp || want_shd) {
        hipStream_t cs = ctx->copy_stream;
        HIPCHK(ctx, hipEventRecord(H.mask_ready, s));
        HIPCHK(ctx, hipStreamWaitEvent(cs, H.mask_ready, 0));
        if (want_shp && gpu_ct) {
            rc = copy_contours(ctx, W, n, H, cs);
            if (rc) return rc;
        } else if (want_shp) {
            HIPCHK(ctx, hipMemcpyAsync(H.h_bits.p, W.d_bits.p, sizeof(uint64_t) * n * h * wpr, hipMemcpyDeviceToHost, cs));
        }
        if (want_shd)
            HIPCHK(ctx, hipMemcpyAsync(H.h_shadow.p, W.d_shadow.p, sizeof(unsigned long long) * 2 * n,
                                       hipMemcpyDeviceToHost, cs));
        HIPCHK(ctx, hipEventRecord(H.mask_done, cs));
        L.mask_reader = &H;
    } else {
        HIPCHK(ctx, hipEventRecord(H.mask_done, s));
    }
    if (want_col) {
        // (n_colors <= 5: the keys in k_uq_part's segmented layout, W.d_raw)
        const bool seg = n_colors <= kMaxK;
        const int64_t cube_stride = std::min<int64_t>(key_stride, kMaxCubes);  // (color_stage's strides)
        const int64_t cell_stride = std::min<int64_t>(cube_stride, (int64_t)kParts * kCellsPerPart);
        const KmeansCubes cubes{W.d_cubes.p, cube_stride, W.d_ncubes.p, W.d_pmeta.p + (size_t)2 * n * kParts, W.d_cells.p,
                                W.d_ncells.p, cell_stride, seg ? W.d_pmeta.p : nullptr, W.d_sups.p, W.d_nsups.p,
                                cell_stride, W.d_pmom.p};
        rc = kmeans_stage(ctx, W, seg ? W.d_raw.p : W.d_keys.p, key_stride, W.d_nuniq.p, n, n_colors, seed, index,
                          cubes, col_s);
        if (rc) return rc;
        HIPCHK(ctx, H.h_kout.ensure(n));
        HIPCHK(ctx, hipMemcpyAsync(H.h_kout.p, W.d_kout.p, sizeof(KmeansImageOut) * n, hipMemcpyDeviceToHost, col_s));
        if (col_s != s) {  // the chunk (and the next chunk's use of this workspace) ends after both
            HIPCHK(ctx, hipEventRecord(ctx->colour_done, col_s));
            HIPCHK(ctx, hipStreamWaitEvent(s, ctx->colour_done, 0));
        }
    }
    HIPCHK(ctx, hipEventRecord(H.chunk_done, s));
    return LLFE_OK;
}

// The shapes and contour counts of a chunk's n images (ctx->img_shapes, ctx->img_ncont) go
// into their result records and, as far as it has room, the caller's shape array.
void emit_shapes(llfe_ctx *ctx, int n, int i0, llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                 int64_t &total_shapes) {
    for (int i = 0; i < n; i++) {
        llfe_image_result &r = results[i0 + i];
        r.shape_offset = total_shapes;
        r.n_shapes = (int32_t)ctx->img_shapes[i].size();
        r.n_contours = ctx->img_ncont[i];
        for (size_t k = 0; k < ctx->img_shapes[i].size(); k++) {
            if (shapes && total_shapes + (int64_t)k < shape_capacity) shapes[total_shapes + k] = ctx->img_shapes[i][k];
        }
        total_shapes += r.n_shapes;
    }
}

}  // namespace

// Shape records of n images from their bit-packed dilated masks (hb, host) on the
// context's thread pool: external contours + the analyze_shapes loop (contours.cpp).
void llfe_host::host_shapes_from_bits(llfe_ctx *ctx, const uint64_t *hb, int n, int h, int w, int i0,
                                      llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                                      int64_t &total_shapes, const llfe_shape_image *ragged) {
    const int wpr = words_per_row(w);
    ctx->img_shapes.resize(n);
    ctx->img_ncont.assign(n, 0);
    const auto t0 = std::chrono::steady_clock::now();
    ctx->pool->parallel_for(n, [&](int i, int wid) {
        if (ragged) {
            const llfe_shape_image &q = ragged[i];
            external_contours_bits(hb + q.word_offset, q.height, q.width, words_per_row(q.width), ctx->work[wid],
                                   ctx->cont[wid]);
        } else {
            external_contours_bits(hb + (size_t)i * h * wpr, h, w, wpr, ctx->work[wid], ctx->cont[wid]);
        }
        ctx->img_ncont[i] = shapes_from_contours(ctx->cont[wid], ctx->shs[wid], ctx->img_shapes[i]);
    });
    ctx->host_ct_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->host_ct_images += n;
    emit_shapes(ctx, n, i0, results, shapes, shape_capacity, total_shapes);
}

namespace {

// A redo of part of a chunk runs synchronously on lane L (lane 0): the device is idle after
// the hipDeviceSynchronize, and the input, staged again without its noise, is still the caller's.
int redo_input(llfe_ctx *ctx, Lane &L, const llfe_batch *b, int i0, int n, const uint8_t **img) {
    HIPCHK(ctx, hipDeviceSynchronize());
    const int8_t *noise;
    llfe_batch nb = *b;
    nb.noise = nullptr;
    return stage_input(ctx, L.W, &nb, i0, n, img, &noise, L.stream);
}

// Recompute the dilated masks of a chunk into lane L's d_bits.
int redo_masks(llfe_ctx *ctx, Lane &L, const llfe_batch *b, int i0, int n) {
    Work &W = L.W;
    hipStream_t s = L.stream;
    const int h = b->height, w = b->width;
    const uint8_t *img;
    int rc = redo_input(ctx, L, b, i0, n, &img);
    if (rc) return rc;
    HIPCHK(ctx, W.d_cls.ensure((size_t)n * h * w));
    HIPCHK(ctx, W.d_bits.ensure((size_t)n * h * words_per_row(w)));
    StencilParams sp;
    if ((rc = stencil_params(ctx, W, n, h, w, s, &sp))) return rc;
    HIPCHK(ctx, launch_stencil(img, n, h, w, W.d_cls.p, nullptr, nullptr, nullptr, nullptr, sp, s));
    return run_hysteresis_dilate(ctx, W, n, h, w, W.d_bits.p, nullptr, s);
}

// Recompute the font bit rows of a chunk into lane L's d_fbits (the input is read through the
// host slot's image table when the chunk was submitted in place).
int redo_font_bits(llfe_ctx *ctx, Lane &L, const llfe_batch *b, int i0, int n, const HostSlot &H, const uint8_t **img) {
    Work &W = L.W;
    const int h = b->height, w = b->width;
    const int rc = redo_input(ctx, L, b, i0, n, img);
    if (rc) return rc;
    HIPCHK(ctx, W.d_fbits.ensure((size_t)n * h * words_per_row(w)));
    HIPCHK(ctx, launch_font_bits(*img, H.img_tab, n, h, w, W.d_fbits.p, L.stream));
    return LLFE_OK;
}

// Font records of a chunk (LLFE_FEATURE_FONTS) from the host slot's copies.  The rare cases
// go the way gpu_shapes_of_chunk's do, so one unusual image never fails its batch: a pass
// that overflowed a contour capacity is redone for this chunk alone, synchronously on
// lane 0, with the capacities grown from what its counters asked for; an image wider
// than 4096 / taller than 65535, or a mask the border follower flags, has its bit rows
// copied back and traced on the host pool (external_contours_bits), boxes, filter and first
// maximum of w * h on the host, and only the gray sums on the device.
int fonts_of_chunk(llfe_ctx *ctx, const llfe_batch *b, int i0, int n, HostSlot &H, llfe_font_result *out) {
    const int h = b->height, w = b->width, wpr = words_per_row(w);
    Lane &L = ctx->lanes[0];
    hipStream_t s = L.stream;
    Work &W = L.W;
    bool host = !H.font_gpu;
    for (int attempt = 0; !host; attempt++) {
        const CtCounters ct = *H.h_font_ctr.p;
        if (ct.flags & ~kCtOverflowMask) {
            host = true;
            break;
        }
        if (!(ct.flags & kCtOverflowMask)) break;
        if (attempt >= 8) return ctx->fail(LLFE_ERR_CAPACITY, "font contours: capacities still overflow (0x%x)", ct.flags);
        const uint8_t *img;
        int rc = redo_font_bits(ctx, L, b, i0, n, H, &img);
        if (rc) return rc;
        grow_contour_caps(W, n, h, w, ct);
        rc = font_pass(ctx, W, img, H.img_tab, n, h, w, H, s);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    if (!host) {
        std::memcpy(out, H.h_font_rec.p, sizeof(llfe_font_result) * (size_t)n);
        return LLFE_OK;
    }
    const uint8_t *img;
    int rc = redo_font_bits(ctx, L, b, i0, n, H, &img);
    if (rc) return rc;
    const size_t words = (size_t)n * h * wpr;
    HIPCHK(ctx, ctx->h_fbits.ensure(words));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_fbits.p, W.d_fbits.p, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    const uint64_t *hb = ctx->h_fbits.p;
    ctx->pool->parallel_for(n, [&](int i, int wid) {
        Contours &c = ctx->cont[wid];
        external_contours_bits(hb + (size_t)i * h * wpr, h, w, wpr, ctx->work[wid], c);
        const int nc = (int)c.start.size() - 1;
        llfe_font_result r{};
        r.n_contours = std::max(nc, 0);
        int64_t best = -1;
        for (int k = 0; k < nc; k++) {  // cv2's list order: newest start first
            const int j = nc - 1 - k;
            int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
            for (int64_t p = c.start[j]; p < c.start[j + 1]; p++) {
                x0 = std::min(x0, c.xy[2 * p]);
                x1 = std::max(x1, c.xy[2 * p]);
                y0 = std::min(y0, c.xy[2 * p + 1]);
                y1 = std::max(y1, c.xy[2 * p + 1]);
            }
            if (x1 < x0) continue;
            const int64_t bw = (int64_t)x1 - x0 + 1, bh = (int64_t)y1 - y0 + 1;
            if (!(10 * bw > bh && bw < 15 * bh && bh > 8)) continue;  // 0.1 < w / float(h) < 15 and h > 8
            r.n_regions++;
            if (bw * bh > best) {  // max(key = w * h): the first maximum wins
                best = bw * bh;
                r.x = x0;
                r.y = y0;
                r.width = (int32_t)bw;
                r.height = (int32_t)bh;
            }
        }
        out[i] = r;
    });
    HIPCHK(ctx, W.d_font_rec.ensure((size_t)n));
    HIPCHK(ctx, hipMemcpyAsync(W.d_font_rec.p, out, sizeof(llfe_font_result) * n, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, launch_font_gray_sum(img, n, h, w, W.d_font_rec.p, s, H.img_tab));
    HIPCHK(ctx, hipMemcpyAsync(out, W.d_font_rec.p, sizeof(llfe_font_result) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->font_fallbacks++;
    return LLFE_OK;
}

// Shape records of a chunk whose contours ran on the GPU (the host slot's copies).  A pass
// that overflowed a capacity is redone for this chunk alone, synchronously on lane 0, with
// the capacities grown from what its counters asked for.  A mask the GPU tracer does not
// handle (a border-following anomaly, a contour wider than its LDS window, a deeper
// Douglas-Peucker stack than it holds) is traced on the host pool instead: the chunk's
// masks are recomputed, copied back and run through the bit-identical host path, so
// one unusual image never fails its batch.
int gpu_shapes_of_chunk(llfe_ctx *ctx, const llfe_batch *b, int i0, int n, HostSlot &H, llfe_image_result *results,
                        llfe_shape *shapes, int64_t shape_capacity, int64_t &total_shapes) {
    const int h = b->height, w = b->width;
    Lane &L = ctx->lanes[0];
    hipStream_t s = L.stream;
    Work &W = L.W;
    for (int attempt = 0;; attempt++) {
        const CtCounters ct = *H.h_ct_ctr.p;
        if ((ct.flags & (kCtBadTrace | kCtTooWide | kCtDpOverflow)) || ctx->force_ct_fallback) {
            int rc = redo_masks(ctx, L, b, i0, n);
            if (rc) return rc;
            const size_t words = (size_t)n * h * words_per_row(w);
            HIPCHK(ctx, H.h_bits.ensure(words));
            HIPCHK(ctx, hipMemcpyAsync(H.h_bits.p, W.d_bits.p, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
            host_shapes_from_bits(ctx, H.h_bits.p, n, h, w, i0, results, shapes, shape_capacity, total_shapes);
            ctx->host_fallbacks++;
            return LLFE_OK;
        }
        if (!(ct.flags & kCtOverflowMask)) break;
        if (attempt >= 8) return ctx->fail(LLFE_ERR_CAPACITY, "GPU contours: capacities still overflow (0x%x)", ct.flags);
        // redo the shapes path of this chunk on lane 0 once the device is idle
        int rc = redo_masks(ctx, L, b, i0, n);
        if (rc) return rc;
        grow_contour_caps(W, n, h, w, ct);
        rc = run_contours(ctx, W, n, h, w, W.d_bits.p, s);
        if (rc) return rc;
        rc = copy_contours(ctx, W, n, H, s);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    const int *info = H.h_ct_info.p;
    const llfe_shape *src = H.h_ct_shapes.p;
    ctx->img_shapes.resize(n);
    ctx->img_ncont.assign(n, 0);
    for (int i = 0; i < n; i++) {
        const int nk = info[i * kCtInfo + 3], sb = info[i * kCtInfo + 4];
        ctx->img_ncont[i] = info[i * kCtInfo + 2];
        ctx->img_shapes[i].assign(src + sb, src + sb + nk);
    }
    emit_shapes(ctx, n, i0, results, shapes, shape_capacity, total_shapes);
    return LLFE_OK;
}

// Host half of one chunk: wait for its host slot, fill the result records, trace contours.
// fonts (LLFE_FEATURE_FONTS): the batch's font records; the chunk's go to fonts[i0 ...]
int finish_chunk(llfe_ctx *ctx, const llfe_batch *b, uint32_t features, int i0, int n, HostSlot &H,
                 llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity, int64_t &total_shapes,
                 llfe_font_result *fonts) {
    const int h = b->height, w = b->width;
    const bool want_col = features & LLFE_FEATURE_COLORS, want_shp = features & LLFE_FEATURE_SHAPES,
               want_shd = features & LLFE_FEATURE_SHADOWS;
    // shapes + shadows are ready first (the GPU may still be in this chunk's colours)
    HIPCHK(ctx, hipEventSynchronize(H.mask_done));
    const unsigned long long *sh = H.h_shadow.p;
    for (int i = 0; i < n; i++) {
        llfe_image_result &r = results[i0 + i];
        std::memset(&r, 0, sizeof r);
        r.shadow_level = -1;
        if (want_shd) {
            r.shadow_sum = sh[i];
            r.shadow_count = sh[n + i];
            r.shadow_level = shadow_level(r.shadow_sum, r.shadow_count);
        }
    }
    if ((features & LLFE_FEATURE_FONTS) && fonts) {
        int rc = fonts_of_chunk(ctx, b, i0, n, H, fonts + i0);
        if (rc) return rc;
    }
    if (want_shp && H.gpu_ct) {
        int rc = gpu_shapes_of_chunk(ctx, b, i0, n, H, results, shapes, shape_capacity, total_shapes);
        if (rc) return rc;
    } else if (want_shp) {
        host_shapes_from_bits(ctx, H.h_bits.p, n, h, w, i0, results, shapes, shape_capacity, total_shapes);
    }
    HIPCHK(ctx, hipEventSynchronize(H.chunk_done));
    if (want_col) {
        const KmeansImageOut *ko = H.h_kout.p;
        for (int i = 0; i < n; i++) fill_color_result(ko[i], results[i0 + i]);
        if (ctx->prof.on) {
            double kb = 0, ub = 0;
            for (int i = 0; i < n; i++) {
                kb += (double)ko[i].bytes;
                ub += 4.0 * (double)ko[i].n_unique;
            }
            ctx->prof.add_bytes("k_kmeans", kb);
            // the unique keys: written once (k_uq_part, 4U of SURVEY.md 8d's 8U) and read
            // once -- by k_uq_gather when it makes them contiguous (n_colors > 5), else by
            // k-means itself where k_uq_part wrote them (its passes' 4U bytes)
            ctx->prof.add_bytes("k_uq_part", ub);
            if ((b->n_colors ? b->n_colors : kMaxK) > kMaxK) ctx->prof.add_bytes("k_uq_gather", ub);
        }
    }
    return LLFE_OK;
}

// The argument checks shared by the batch entry points (have_data: n == 0 or a data pointer).
// submit_fn: the submitting entry point, whose batch must fit one device pass (else null).
int check_batch_args(llfe_ctx *ctx, int n, int h, int w, bool have_data, int n_colors, const char *submit_fn = nullptr) {
    if (!valid_dims(n, h, w) || !have_data)
        return ctx->fail(LLFE_ERR_INVALID, "invalid batch n=%d h=%d w=%d", n, h, w);
    if (n_colors < 0 || n_colors > kMaxColors)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "n_colors=%d outside [1, %d]", n_colors, kMaxColors);
    if (submit_fn && n > chunk_for(h, w))
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "%s: n=%d exceeds one device pass (%d)", submit_fn, n, chunk_for(h, w));
    return LLFE_OK;
}

// Claim the next ticket's host slot and lane (the submit path uses lane == slot), refused
// while the slot's previous ticket is not collected; the lane's stream then waits for the
// caller's stream (inputs produced there).
int claim_ticket_slot(llfe_ctx *ctx, llfe_stream stream, int *slot) {
    *slot = (int)(ctx->next_ticket % ctx->inflight_max);
    if (ctx->slots[*slot].pending.busy)
        return ctx->fail(LLFE_ERR_CAPACITY, "%d batches already in flight: collect one first", ctx->inflight_max);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventRecord(ctx->start_ev, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->lanes[*slot].stream, ctx->start_ev, 0));
    return LLFE_OK;
}

// the enqueued batch becomes the next ticket
void publish_ticket(llfe_ctx *ctx, Pending &pd, const llfe_batch &b, uint32_t features, int64_t *ticket) {
    pd.busy = true;
    pd.done = false;
    pd.b = b;
    pd.features = features;
    *ticket = ctx->next_ticket++;
}

}  // namespace

extern "C" {

int llfe_process_batch(llfe_ctx *ctx, const llfe_batch *b, uint32_t features, uint64_t seed,
                       llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                       int64_t *shapes_needed, llfe_stream stream) {
    if (!ctx || !b || !results) return LLFE_ERR_INVALID;
    if (int rc_ = check_batch_args(ctx, b->n, b->height, b->width, b->n == 0 || b->data, b->n_colors)) return rc_;
    if (ctx->any_inflight())
        return ctx->fail(LLFE_ERR_INVALID, "llfe_process_batch with submitted batches not yet collected");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const bool want_shp = features & LLFE_FEATURE_SHAPES;
    int64_t total_shapes = 0;
    ctx->font_has = false;  // (llfe_font_records: the previous call's records end here)
    ctx->font_recs.assign((features & LLFE_FEATURE_FONTS) ? (size_t)b->n : 0, llfe_font_result{});
    llfe_font_result *const fonts = ctx->font_recs.data();
    // two-slot software pipeline: enqueue chunk c on lane 0 (its workspace and streams; the
    // D2H goes into host slot c & 1), then finish chunk c - 1 on the host (contours, result
    // records) from host slot (c - 1) & 1 while the GPU runs c.  Every lane's stream first
    // waits for the caller's stream (inputs produced there).
    HIPCHK(ctx, hipEventRecord(ctx->start_ev, s));
    for (Lane &L : ctx->lanes) HIPCHK(ctx, hipStreamWaitEvent(L.stream, ctx->start_ev, 0));
    int prev_i0 = -1, prev_n = 0, slot = 0;
    auto finish_prev = [&](HostSlot &H) {  // (nothing before the first chunk)
        return prev_i0 < 0 ? LLFE_OK : finish_chunk(ctx, b, features, prev_i0, prev_n, H, results, shapes, shape_capacity,
                                                    total_shapes, fonts);
    };
    const int chunk = chunk_for(b->height, b->width);
    for (int i0 = 0; i0 < b->n; i0 += chunk) {
        const int n = std::min(chunk, b->n - i0);
        int rc = enqueue_chunk(ctx, b, features, seed, i0, n, ctx->lanes[0], ctx->slots[slot], slot);
        if (rc) return rc;
        if ((rc = finish_prev(ctx->slots[slot ^ 1]))) return rc;
        prev_i0 = i0;
        prev_n = n;
        slot ^= 1;
    }
    if (int rc = finish_prev(ctx->slots[slot ^ 1])) return rc;
    // (every chunk has been waited for; the caller's stream gets the same order)
    for (int q = 0; q < 2; q++) {
        HIPCHK(ctx, hipEventRecord(ctx->lanes[q].stream_done, ctx->lanes[q].stream));
        HIPCHK(ctx, hipStreamWaitEvent(s, ctx->lanes[q].stream_done, 0));
    }
    ctx->prof.collect();
    ctx->font_owner = LLFE_LAST_CALL;
    ctx->font_has = (features & LLFE_FEATURE_FONTS) != 0;
    if (shapes_needed) *shapes_needed = total_shapes;
    if (want_shp && total_shapes > shape_capacity)
        return ctx->fail(LLFE_ERR_CAPACITY, "shape capacity %lld < %lld", (long long)shape_capacity,
                         (long long)total_shapes);
    return LLFE_OK;
}

}  // extern "C"

// llfe_process_images (its entry points are in llfe_colors_images.cpp).
// Ragged batch: images grouped by (preprocessed) size in input order; each group is
// packed into a device buffer (2-D copies absorb row strides and host / device sources;
// images the preprocessing rule resizes go through cv2.resize on the GPU) and runs as
// ordinary batches that carry every image's own global index.
int llfe_host::process_images_grouped(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                                      int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                                      llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                                      int64_t *shapes_needed, llfe_stream stream) {
    if (!ctx || n < 0 || (n > 0 && (!images || !results))) return LLFE_ERR_INVALID;
    if (preprocessing < LLFE_PRE_NONE || preprocessing > LLFE_PRE_PERFORMANCE)
        return ctx->fail(LLFE_ERR_INVALID, "preprocessing mode %d", preprocessing);
    if (n_colors < 0 || n_colors > kMaxColors)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "n_colors=%d outside [1, %d]", n_colors, kMaxColors);
    if (ctx->any_inflight())
        return ctx->fail(LLFE_ERR_INVALID, "llfe_process_images with submitted batches not yet collected");
    struct Item {
        int oh, ow, interp;
        bool resize;
    };
    std::vector<Item> it((size_t)n);
    const bool with_noise = n > 0 && images[0].noise;
    for (int i = 0; i < n; i++) {
        const llfe_image_desc &d = images[i];
        if (!d.data || !valid_dims(1, d.height, d.width) ||
            (d.row_stride != 0 && d.row_stride < 3 * (int64_t)d.width))
            return ctx->fail(LLFE_ERR_INVALID, "image %d: invalid descriptor (%d x %d, stride %lld)", i, d.height,
                             d.width, (long long)d.row_stride);
        if ((d.noise != nullptr) != with_noise)
            return ctx->fail(LLFE_ERR_INVALID, "parity noise must be given for every image or for none");
        Item &q = it[i];
        int ow = d.width, oh = d.height, interp = 0;
        const int r = llfe_preprocess_size(d.width, d.height, preprocessing, &ow, &oh, &interp);
        if (r < 0) return ctx->fail(LLFE_ERR_INVALID, "image %d: preprocessing size", i);
        q = Item{r ? oh : d.height, r ? ow : d.width, interp, r == 1};
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    // size groups, in order of first appearance; members in input order
    std::vector<std::pair<std::pair<int, int>, std::vector<int>>> groups;
    {
        std::map<std::pair<int, int>, size_t> gi;
        for (int i = 0; i < n; i++) {
            const auto key = std::make_pair(it[i].oh, it[i].ow);
            auto f = gi.find(key);
            if (f == gi.end()) {
                gi[key] = groups.size();
                groups.push_back({key, {i}});
            } else {
                groups[f->second].second.push_back(i);
            }
        }
    }
    const bool want_shp = features & LLFE_FEATURE_SHAPES, want_fnt = features & LLFE_FEATURE_FONTS;
    int64_t total_shapes = 0;
    bool short_cap = false;
    ctx->font_has = false;
    std::vector<llfe_font_result> fonts(want_fnt ? (size_t)n : 0);  // in input order (each group's call leaves its own)
    std::vector<llfe_image_result> res;
    std::vector<int64_t> gidx;
    for (const auto &g : groups) {
        const int oh = g.first.first, ow = g.first.second;
        const int64_t P3 = (int64_t)oh * ow * 3;
        // staging passes of at most two device chunks (the batch path pipelines them)
        const int per = std::max(1, 2 * chunk_for(oh, ow));
        for (size_t a = 0; a < g.second.size(); a += per) {
            const int nb = (int)std::min<size_t>(per, g.second.size() - a);
            HIPCHK(ctx, ctx->d_ragged.ensure((size_t)nb * P3));
            if (with_noise) HIPCHK(ctx, ctx->d_ragged_noise.ensure((size_t)nb * P3));
            gidx.resize(nb);
            for (int j = 0; j < nb; j++) {
                const int i = g.second[a + j];
                const llfe_image_desc &d = images[i];
                gidx[j] = index_base + i;
                const size_t pitch = d.row_stride ? (size_t)d.row_stride : (size_t)d.width * 3;
                const hipMemcpyKind kind = d.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
                uint8_t *dst = ctx->d_ragged.p + (size_t)j * P3;
                if (!it[i].resize) {
                    HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)ow * 3, d.data, pitch, (size_t)d.width * 3, d.height,
                                                 kind, s));
                } else {
                    HIPCHK(ctx, ctx->d_rsz_src.ensure((size_t)d.height * d.width * 3));
                    HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_rsz_src.p, (size_t)d.width * 3, d.data, pitch,
                                                 (size_t)d.width * 3, d.height, kind, s));
                    const int rc = llfe_resize_cv(ctx, ctx->d_rsz_src.p, d.height, d.width, 3, dst, oh, ow,
                                                  it[i].interp, stream);
                    if (rc) return rc;
                }
                if (with_noise)
                    HIPCHK(ctx, hipMemcpyAsync(ctx->d_ragged_noise.p + (size_t)j * P3, d.noise, (size_t)P3,
                                               d.noise_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
            }
            llfe_batch bb{};
            bb.data = ctx->d_ragged.p;
            bb.n = nb;
            bb.height = oh;
            bb.width = ow;
            bb.on_device = 1;
            bb.noise = with_noise ? ctx->d_ragged_noise.p : nullptr;
            bb.noise_on_device = 1;
            bb.n_colors = n_colors;
            bb.index_base = index_base;
            bb.indices = gidx.data();
            res.assign((size_t)nb, llfe_image_result{});
            const int64_t left = std::max<int64_t>(0, shape_capacity - total_shapes);
            int64_t need = 0;
            const int rc = llfe_process_batch(ctx, &bb, features, seed, res.data(),
                                              shapes && left > 0 ? shapes + total_shapes : nullptr, left, &need,
                                              stream);
            if (rc == LLFE_ERR_CAPACITY) {
                short_cap = true;  // results are valid; keep counting what is needed
            } else if (rc) {
                return rc;
            }
            for (int j = 0; j < nb; j++) {
                llfe_image_result r = res[j];
                r.shape_offset += total_shapes;
                results[g.second[a + j]] = r;
                if (want_fnt) fonts[g.second[a + j]] = ctx->font_recs[j];
            }
            total_shapes += need;
        }
    }
    ctx->font_recs.swap(fonts);
    ctx->font_owner = LLFE_LAST_CALL;
    ctx->font_has = want_fnt;
    if (shapes_needed) *shapes_needed = total_shapes;
    if (want_shp && (short_cap || total_shapes > shape_capacity))
        return ctx->fail(LLFE_ERR_CAPACITY, "shape capacity %lld < %lld", (long long)shape_capacity,
                         (long long)total_shapes);
    return LLFE_OK;
}

extern "C" {

// Asynchronous form of llfe_process_batch: up to two batches in flight, each on its own
// lane and host slot, so batch k + 1's unique-colour and stencil kernels start in
// the tail of batch k's k-means launch (where most CUs are idle) instead of after it.
int llfe_submit_batch(llfe_ctx *ctx, const llfe_batch *b, uint32_t features, uint64_t seed, llfe_stream stream,
                      int64_t *ticket) {
    if (!ctx || !b || !ticket) return LLFE_ERR_INVALID;
    if (int rc_ = check_batch_args(ctx, b->n, b->height, b->width, b->n == 0 || b->data, b->n_colors, __func__)) return rc_;
    int slot;
    if (int rc_ = claim_ticket_slot(ctx, stream, &slot)) return rc_;
    if (b->n > 0) {
        int rc = enqueue_chunk(ctx, b, features, seed, 0, b->n, ctx->lanes[slot], ctx->slots[slot], slot);
        if (rc) return rc;
    }
    publish_ticket(ctx, ctx->slots[slot].pending, *b, features, ticket);
    return LLFE_OK;
}

// The request path's micro-batch (MicroBatcher): separately allocated images of one size
// gathered into the lane's input buffer on the lane's stream, then the same device work
// as llfe_submit_batch, every image under its own global index.
int llfe_submit_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features, int32_t n_colors,
                       uint64_t seed, const int64_t *indices, llfe_stream stream, int64_t *ticket) {
    if (!ctx || !ticket || n < 1 || !images || !indices) return LLFE_ERR_INVALID;
    const int h = images[0].height, w = images[0].width;
    if (int rc_ = check_batch_args(ctx, n, h, w, true, n_colors, __func__)) return rc_;
    int nd = 0;
    for (int i = 0; i < n; i++) {
        const llfe_image_desc &d = images[i];
        if (!d.data || d.height != h || d.width != w || (d.row_stride != 0 && d.row_stride < 3 * (int64_t)w))
            return ctx->fail(LLFE_ERR_INVALID, "image %d: %d x %d stride %lld in a %d x %d submission", i, d.height,
                             d.width, (long long)d.row_stride, h, w);
        if (d.noise)
            return ctx->fail(LLFE_ERR_UNSUPPORTED, "image %d: parity noise goes through llfe_process_images", i);
        nd += d.on_device ? 1 : 0;
    }
    int slot;
    if (int rc_ = claim_ticket_slot(ctx, stream, &slot)) return rc_;
    Lane &L = ctx->lanes[slot];
    HostSlot &H = ctx->slots[slot];
    hipStream_t q = L.stream;
    Work &W = L.W;
    const size_t P3 = (size_t)h * w * 3;
    ctx->prof.cur_slot = slot;
    // in place when every image is a packed, 16-B aligned device image: the scatter and the
    // stencil (the only readers of the input) take image i's address from a table; else (host
    // sources, strided rows, the GPU contour mode, whose capacity redo re-reads a packed
    // batch) the images are gathered into the lane's input buffer first
    bool in_place = nd == n && !ctx->gpu_contours;
    for (int i = 0; in_place && i < n; i++)
        in_place = (images[i].row_stride == 0 || images[i].row_stride == 3 * (int64_t)w) &&
                   (((uintptr_t)images[i].data) & 15) == 0;
    const uint64_t *d_tab = nullptr;
    if (nd == n) {
        // a table of addresses and pitches (pinned, per host slot: the slot is not reused before
        // this ticket's collect), then one gather launch unless the kernels read in place
        HIPCHK(ctx, H.h_gather.ensure(2 * (size_t)n));
        HIPCHK(ctx, H.d_gather.ensure(2 * (size_t)n));
        uint64_t *tab = H.h_gather.p;
        for (int i = 0; i < n; i++) {
            tab[i] = (uint64_t)(uintptr_t)images[i].data;
            tab[n + i] = (uint64_t)(images[i].row_stride ? images[i].row_stride : 3 * (int64_t)w);
        }
        HIPCHK(ctx, hipMemcpyAsync(H.d_gather.p, tab, sizeof(uint64_t) * 2 * n, hipMemcpyHostToDevice, q));
        if (in_place) {
            d_tab = H.d_gather.p;
        } else {
            HIPCHK(ctx, W.d_in.ensure(P3 * n));
            TIMED(ctx, q, "k_gather_images", 2.0 * (double)P3 * n, launch_gather_images(H.d_gather.p, n, h, w, W.d_in.p, q));
        }
    } else {
        HIPCHK(ctx, W.d_in.ensure(P3 * n));
        for (int i = 0; i < n; i++) {
            const llfe_image_desc &d = images[i];
            const size_t pitch = d.row_stride ? (size_t)d.row_stride : (size_t)w * 3;
            HIPCHK(ctx, hipMemcpy2DAsync(W.d_in.p + (size_t)i * P3, (size_t)w * 3, d.data, pitch, (size_t)w * 3, h,
                                         d.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, q));
        }
    }
    Pending &pd = H.pending;
    pd.idx.assign(indices, indices + n);
    llfe_batch b{};
    b.data = d_tab ? images[0].data : W.d_in.p;
    b.n = n;
    b.height = h;
    b.width = w;
    b.on_device = 1;
    b.n_colors = n_colors;
    b.indices = pd.idx.data();
    int rc = enqueue_chunk(ctx, &b, features, seed, 0, n, L, H, slot, d_tab);
    if (rc) return rc;
    publish_ticket(ctx, pd, b, features, ticket);
    return LLFE_OK;
}

int llfe_collect_batch(llfe_ctx *ctx, int64_t ticket, llfe_image_result *results, llfe_shape *shapes,
                       int64_t shape_capacity, int64_t *shapes_needed) {
    if (!ctx || !results) return LLFE_ERR_INVALID;
    if (ticket != ctx->next_collect) return ctx->fail(LLFE_ERR_INVALID, "collect tickets in submission order");
    const int slot = (int)(ticket % ctx->inflight_max);
    HostSlot &H = ctx->slots[slot];
    Pending &pd = H.pending;
    if (!pd.busy) return ctx->fail(LLFE_ERR_INVALID, "ticket %lld was not submitted", (long long)ticket);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int n = pd.b.n;
    if (!pd.done) {  // host half once; a retry after LLFE_ERR_CAPACITY only copies
        pd.res.assign((size_t)n, llfe_image_result{});
        int64_t total = 0;
        if (n > 0) {
            pd.fnt.assign((pd.features & LLFE_FEATURE_FONTS) ? (size_t)n : 0, llfe_font_result{});
            int rc = finish_chunk(ctx, &pd.b, pd.features, 0, n, H, pd.res.data(), nullptr, 0, total, pd.fnt.data());
            if (rc) return rc;
        } else {
            pd.fnt.clear();
        }
        pd.shp.clear();
        if (pd.features & LLFE_FEATURE_SHAPES) {
            pd.shp.reserve((size_t)total);
            // finish_chunk left the per-image shapes in ctx->img_shapes
            for (int i = 0; i < n; i++)
                pd.shp.insert(pd.shp.end(), ctx->img_shapes[i].begin(), ctx->img_shapes[i].end());
        }
        ctx->prof.collect(slot);
        pd.done = true;
    }
    const int64_t total = (int64_t)pd.shp.size();
    if (shapes_needed) *shapes_needed = total;
    std::memcpy(results, pd.res.data(), sizeof(llfe_image_result) * (size_t)n);
    if (shapes) std::memcpy(shapes, pd.shp.data(), sizeof(llfe_shape) * (size_t)std::min(total, shape_capacity));
    if (total > shape_capacity)
        return ctx->fail(LLFE_ERR_CAPACITY, "shape capacity %lld < %lld", (long long)shape_capacity, (long long)total);
    pd.busy = false;
    ctx->next_collect++;
    ctx->font_recs.swap(pd.fnt);
    ctx->font_owner = ticket;
    ctx->font_has = (pd.features & LLFE_FEATURE_FONTS) != 0;
    return LLFE_OK;
}

int llfe_font_records(llfe_ctx *ctx, int64_t ticket, llfe_font_result *out, int32_t n) {
    if (!ctx || !out || n < 0) return LLFE_ERR_INVALID;
    if (!ctx->font_has || ticket != ctx->font_owner)
        return ctx->fail(LLFE_ERR_INVALID, "llfe_font_records: no font records of ticket %lld (not collected, expired, "
                                           "or run without LLFE_FEATURE_FONTS)", (long long)ticket);
    if ((size_t)n != ctx->font_recs.size())
        return ctx->fail(LLFE_ERR_INVALID, "llfe_font_records: n=%d, the call had %zu images", n, ctx->font_recs.size());
    if (n) std::memcpy(out, ctx->font_recs.data(), sizeof(llfe_font_result) * (size_t)n);
    return LLFE_OK;
}

}  // extern "C"
