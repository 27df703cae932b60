// The shapes and shadows of a batch of images of any sizes in one device pass
// (LLFE_IMAGES_SHAPES_ONE_PASS of llfe_process_images_routes, llfe_shape_bits_images,
// llfe_shadow_stats_images, llfe_hysteresis_images): the host planner, the staging of the images
// that cannot be read where they lie, and the pass itself -- the ragged stencil over per-image
// records and a work table (stencil_stream.hip), the ragged hysteresis and dilate over a tile
// table (hysteresis.hip), one D2H of every mask word and shadow sum, and one fan-out of the
// images over the host contour pool.
#include "llfe_ctx.h"

using namespace llfe_host;

namespace {

constexpr int64_t kMaxPassTiles = (int64_t(1) << 31) / 4096;  // the ids tile * 4096 + node are int
constexpr int64_t kTileBytes = 4096 * 7 + 512 + 20;  // parent, sroot, roots; tstrong; counts, lists, flags

struct ShapePlan {
    std::vector<llfe_shape_image> img;
    std::vector<llfe_shape_work> work;
    std::vector<llfe_shape_pass> pass;
    std::vector<int> interp;  // cv2 interpolation of the images the rule resizes
};

inline int64_t align16(int64_t x) { return (x + 15) & ~int64_t(15); }

bool read_in_place(const llfe_image_desc &d, const llfe_shape_image &r) {
    return d.on_device && !r.resized && (d.row_stride == 0 || d.row_stride == 3 * (int64_t)d.width);
}

int64_t workspace_bytes(const llfe_shape_pass &p, int64_t work_count) {
    return 3 * p.class_bytes + kTileBytes * p.tiles + 16 * p.words + p.stage_bytes + 8 * work_count;
}

// -> LLFE_OK, or LLFE_ERR_INVALID with *bad = the image (or -1: the arguments)
int plan_shapes(const llfe_image_desc *descs, int n, int preprocessing, ShapePlan &pl, int *bad) {
    *bad = -1;
    if (n < 0 || (n > 0 && !descs) || preprocessing < LLFE_PRE_NONE || preprocessing > LLFE_PRE_PERFORMANCE)
        return LLFE_ERR_INVALID;
    pl.img.assign((size_t)n, llfe_shape_image{});
    pl.interp.assign((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const llfe_image_desc &d = descs[i];
        *bad = i;
        if (!d.data || !valid_dims(1, d.height, d.width) || (d.row_stride != 0 && d.row_stride < 3 * (int64_t)d.width))
            return LLFE_ERR_INVALID;
        int ow = d.width, oh = d.height, interp = 0;
        const int r = llfe_preprocess_size(d.width, d.height, preprocessing, &ow, &oh, &interp);
        if (r < 0) return LLFE_ERR_INVALID;
        llfe_shape_image &q = pl.img[i];
        q.height = r ? oh : d.height;
        q.width = r ? ow : d.width;
        q.resized = r == 1;
        q.pixels = (int64_t)q.height * q.width;
        stencil_stream_geometry(q.height, q.width, &q.strips, &q.segs, &q.seg_rows);
        q.tiles_x = (q.width + 63) >> 6;
        q.tiles_y = (q.height + 63) >> 6;
        q.stage_offset = -1;
        pl.interp[i] = interp;
    }
    *bad = -1;
    const double budget = workspace_gb() * 1e9;
    int64_t first_word = 0;
    for (int i = 0; i < n;) {
        llfe_shape_pass p{};
        p.first = i;
        p.work_first = (int32_t)pl.work.size();
        p.first_word = first_word;
        int64_t waves = 0;
        for (; i < n; i++) {
            llfe_shape_image &q = pl.img[i];
            const int64_t tiles = (int64_t)q.tiles_x * q.tiles_y, w = (int64_t)q.strips * q.segs;
            if (p.count > 0 && p.tiles + tiles >= kMaxPassTiles) break;
            llfe_shape_pass t = p;  // the pass with this image
            t.count = p.count + 1;
            t.tiles = (int32_t)(p.tiles + tiles);
            t.class_bytes = align16(p.class_bytes + q.pixels);
            t.words = p.words + (int64_t)q.height * ((q.width + 63) >> 6);
            const bool staged = !read_in_place(descs[i], q);
            if (staged) t.stage_bytes = align16(p.stage_bytes + q.pixels * 3);
            if (p.count > 0 && (double)workspace_bytes(t, waves + w) > budget) break;
            q.pass = (int32_t)pl.pass.size();
            q.class_offset = p.class_bytes;
            q.word_offset = p.words;
            q.first_tile = p.tiles;
            q.first_part = (int32_t)waves;
            if (staged) q.stage_offset = p.stage_bytes;
            for (int sg = 0; sg < q.segs; sg++)
                for (int st = 0; st < q.strips; st++) pl.work.push_back(llfe_shape_work{i, st, sg});
            p = t;
            waves += w;
        }
        p.work_count = (int32_t)waves;
        p.workspace_bytes = workspace_bytes(p, waves);
        first_word += p.words;
        pl.pass.push_back(p);
    }
    return LLFE_OK;
}

int bad_plan(llfe_ctx *ctx, const llfe_image_desc *images, int bad, int preprocessing) {
    return bad < 0 ? ctx->fail(LLFE_ERR_INVALID, "preprocessing mode %d", preprocessing)
                   : ctx->fail(LLFE_ERR_INVALID, "image %d: invalid descriptor (%d x %d, stride %lld)", bad,
                               images[bad].height, images[bad].width, (long long)images[bad].row_stride);
}

// The tables of pass k in pinned memory and on the device: the records (src filled by the
// caller through `recs`), the work table, the image of every tile.
struct PassTables {
    ShapeImgRec *recs;  // pinned
    ShapeImages dev;
};

int pass_tables(llfe_ctx *ctx, const ShapePlan &pl, int k, PassTables *out) {
    const llfe_shape_pass &p = pl.pass[k];
    const size_t rec_bytes = sizeof(ShapeImgRec) * (size_t)p.count,
                 work_bytes = (size_t)align16((int64_t)(sizeof(ShapeWork) * (size_t)p.work_count)),
                 tile_bytes = sizeof(int32_t) * (size_t)p.tiles, bytes = rec_bytes + work_bytes + tile_bytes;
    HIPCHK(ctx, ctx->h_shape_tab.ensure(bytes));
    HIPCHK(ctx, ctx->d_shape_tab.ensure(bytes));
    ShapeImgRec *recs = (ShapeImgRec *)ctx->h_shape_tab.p;
    ShapeWork *work = (ShapeWork *)(ctx->h_shape_tab.p + rec_bytes);
    int32_t *timg = (int32_t *)(ctx->h_shape_tab.p + rec_bytes + work_bytes);
    for (int j = 0; j < p.count; j++) {
        const llfe_shape_image &q = pl.img[(size_t)p.first + j];
        ShapeImgRec &r = recs[j];
        r = ShapeImgRec{nullptr, q.class_offset, q.word_offset, q.height, q.width, q.strips, q.segs, q.seg_rows, 0,
                        q.tiles_x, q.first_tile, q.first_part, 0};
        std::fill(timg + q.first_tile, timg + q.first_tile + q.tiles_x * q.tiles_y, j);
    }
    for (int e = 0; e < p.work_count; e++) {
        const llfe_shape_work &wk = pl.work[(size_t)p.work_first + e];
        work[e] = ShapeWork{wk.image - p.first, wk.strip, wk.seg};
    }
    uint8_t *d = ctx->d_shape_tab.p;
    out->recs = recs;
    out->dev = ShapeImages{(const ShapeImgRec *)d, (const ShapeWork *)(d + rec_bytes),
                           (const int32_t *)(d + rec_bytes + work_bytes), p.count, p.work_count, p.tiles,
                           p.class_bytes, p.words};
    return LLFE_OK;
}

int upload_tables(llfe_ctx *ctx, const llfe_shape_pass &p, hipStream_t s) {
    const size_t bytes = sizeof(ShapeImgRec) * (size_t)p.count +
                         (size_t)align16((int64_t)(sizeof(ShapeWork) * (size_t)p.work_count)) +
                         sizeof(int32_t) * (size_t)p.tiles;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_shape_tab.p, ctx->h_shape_tab.p, bytes, hipMemcpyHostToDevice, s));
    return LLFE_OK;
}

// The hysteresis workspace of a ragged pass on W (hyst_work's buffers, sized by the pass's
// tiles, class map and words); tflag: the stencil's flags in W.d_tflag, or null.
int hyst_work_images(llfe_ctx *ctx, Work &W, const llfe_shape_pass &p, bool tflag, HystWork *out) {
    const size_t tiles = (size_t)p.tiles, ids = tiles * 4096;
    HIPCHK(ctx, W.d_lab.ensure((size_t)p.class_bytes));
    HIPCHK(ctx, W.d_parent.ensure(ids));
    HIPCHK(ctx, W.d_sroot.ensure(ids));
    HIPCHK(ctx, W.d_roots.ensure(ids));
    HIPCHK(ctx, W.d_nroots.ensure(tiles));
    HIPCHK(ctx, W.d_tstrong.ensure(tiles * hysteresis_tile_words()));
    HIPCHK(ctx, W.d_ebits.ensure((size_t)p.words));
    HIPCHK(ctx, W.d_ftlist.ensure(tiles + 2));
    HIPCHK(ctx, W.d_ptlist.ensure(tiles + 1));
    *out = HystWork{W.d_lab.p,   W.d_parent.p, W.d_sroot.p, W.d_roots.p,       W.d_nroots.p, W.d_tstrong.p,
                    W.d_ebits.p, tflag ? W.d_tflag.p : nullptr, W.d_ftlist.p + 2, W.d_ftlist.p, W.d_ptlist.p};
    W.tflag_valid = false;
    return LLFE_OK;
}

// Device work of pass k on lane 0's workspace and stream s: stage what cannot be read in place,
// one upload of the records and tables, the ragged stencil, then (want_shp) hysteresis and
// dilate into W.d_bits.  The shadow sums are in W.d_shadow (count sums, then count counts).
int shapes_pass_device(llfe_ctx *ctx, const llfe_image_desc *descs, const ShapePlan &pl, int k, bool want_shp,
                       bool want_shd, hipStream_t s) {
    const llfe_shape_pass &p = pl.pass[k];
    Work &W = ctx->lanes[0].W;
    const int slot = ctx->prof.cur_slot;
    HIPCHK(ctx, ctx->d_shape_stage.ensure((size_t)std::max<int64_t>(p.stage_bytes, 16)));
    if (want_shp) HIPCHK(ctx, W.d_cls.ensure((size_t)std::max<int64_t>(p.class_bytes, 16)));
    PassTables tb;
    if (int rc = pass_tables(ctx, pl, k, &tb)) return rc;
    for (int j = p.first; j < p.first + p.count; j++) {
        const llfe_image_desc &d = descs[j];
        const llfe_shape_image &q = pl.img[j];
        const uint8_t *src = d.data;
        if (q.stage_offset >= 0) {
            uint8_t *dst = ctx->d_shape_stage.p + q.stage_offset;
            const size_t pitch = d.row_stride ? (size_t)d.row_stride : (size_t)d.width * 3;
            const hipMemcpyKind kind = d.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
            if (!q.resized) {
                HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)d.width * 3, d.data, pitch, (size_t)d.width * 3, d.height, kind, s));
            } else {
                HIPCHK(ctx, ctx->d_rsz_src.ensure((size_t)d.height * d.width * 3));
                HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_rsz_src.p, (size_t)d.width * 3, d.data, pitch, (size_t)d.width * 3,
                                             d.height, kind, s));
                const int rc = llfe_resize_cv(ctx, ctx->d_rsz_src.p, d.height, d.width, 3, dst, q.height, q.width,
                                              pl.interp[j], (llfe_stream)s);
                if (rc) return rc;
            }
            src = dst;
        }
        ShapeImgRec &r = tb.recs[j - p.first];
        r.src = src;
        // the dword paths of the stencil, decided per image: its own source address, its own
        // class-map address and 3 * W all 4-byte aligned
        const uintptr_t cmap = want_shp ? (uintptr_t)(W.d_cls.p + q.class_offset) : 0;
        r.vec = ((((uintptr_t)src | cmap) & 3) == 0 && (q.width & 3) == 0) ? 1 : 0;
    }
    if (int rc = upload_tables(ctx, p, s)) return rc;
    ctx->prof.cur_slot = slot;  // (a staging resize tags its own records)
    bool flags = want_shp;
    if (const char *e = getenv("LLFE_HYST_TILE_FLAGS"))  // (as stencil_params)
        if (!strcmp(e, "0")) flags = false;
    if (flags) {
        HIPCHK(ctx, W.d_tflag.ensure((size_t)p.tiles));
        HIPCHK(ctx, hipMemsetAsync(W.d_tflag.p, 0, (size_t)p.tiles, s));
    }
    HIPCHK(ctx, W.d_shadow.ensure(2 * (size_t)p.count + (size_t)p.work_count));
    double pixels = 0;
    for (int j = p.first; j < p.first + p.count; j++) pixels += (double)pl.img[j].pixels;
    TIMED(ctx, s, "k_stencil", pixels * (3 + (want_shp ? 1 : 0)),
          launch_stencil_images(tb.dev, want_shp ? W.d_cls.p : nullptr, want_shd ? W.d_shadow.p : nullptr,
                                want_shd ? W.d_shadow.p + p.count : nullptr, (uint2 *)(W.d_shadow.p + 2 * p.count),
                                flags ? W.d_tflag.p : nullptr, s));
    if (want_shp) {
        HystWork wk;
        if (int rc = hyst_work_images(ctx, W, p, flags, &wk)) return rc;
        HIPCHK(ctx, W.d_bits.ensure((size_t)p.words));
        TIMED(ctx, s, "k_hysteresis_dilate", pixels * (1 + 0.125),
              launch_hysteresis_dilate_images(W.d_cls.p, tb.dev, wk, W.d_bits.p, s));
    }
    return LLFE_OK;
}

// ... and the D2H of its mask words and shadow sums into host slot 0 on the copy stream; the
// event H.mask_done says they have arrived (and that lane 0's workspace may be reused)
int shapes_pass_copy(llfe_ctx *ctx, const llfe_shape_pass &p, bool want_shp, bool want_shd, hipStream_t s) {
    Lane &L = ctx->lanes[0];
    HostSlot &H = ctx->slots[0];
    Work &W = L.W;
    hipStream_t cs = ctx->copy_stream;
    if (want_shp) HIPCHK(ctx, H.h_bits.ensure((size_t)p.words));
    if (want_shd) HIPCHK(ctx, H.h_shadow.ensure(2 * (size_t)p.count));
    HIPCHK(ctx, hipEventRecord(H.mask_ready, s));
    HIPCHK(ctx, hipStreamWaitEvent(cs, H.mask_ready, 0));
    if (want_shp)
        HIPCHK(ctx, hipMemcpyAsync(H.h_bits.p, W.d_bits.p, sizeof(uint64_t) * (size_t)p.words, hipMemcpyDeviceToHost, cs));
    if (want_shd)
        HIPCHK(ctx, hipMemcpyAsync(H.h_shadow.p, W.d_shadow.p, sizeof(unsigned long long) * 2 * (size_t)p.count,
                                   hipMemcpyDeviceToHost, cs));
    HIPCHK(ctx, hipEventRecord(H.mask_done, cs));
    L.mask_reader = &H;
    return LLFE_OK;
}

// the checks the stage calls share; -> the plan
int stage_plan(llfe_ctx *ctx, const char *fn, const llfe_image_desc *descs, int n, ShapePlan &pl) {
    if (int rc_ = stage_enter(ctx, fn)) return rc_;
    int bad;
    if (plan_shapes(descs, n, LLFE_PRE_NONE, pl, &bad)) return ctx->fail(LLFE_ERR_INVALID, "image %d: invalid descriptor", bad);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return LLFE_OK;
}

// a stage call's pass on the caller's stream, waited for
int stage_pass(llfe_ctx *ctx, const llfe_image_desc *descs, const ShapePlan &pl, int k, bool want_shp, bool want_shd,
               hipStream_t s) {
    Lane &L = ctx->lanes[0];
    if (L.mask_reader) HIPCHK(ctx, hipStreamWaitEvent(s, L.mask_reader->mask_done, 0));
    if (int rc = shapes_pass_device(ctx, descs, pl, k, want_shp, want_shd, s)) return rc;
    if (int rc = shapes_pass_copy(ctx, pl.pass[k], want_shp, want_shd, s)) return rc;
    HIPCHK(ctx, hipEventSynchronize(ctx->slots[0].mask_done));
    return LLFE_OK;
}

}  // namespace

int llfe_host::process_images_shapes_one_pass(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                                              int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                                              llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                                              int64_t *shapes_needed, llfe_stream stream) {
    // the grouped route's checks, before any work
    if (!ctx || n < 0 || (n > 0 && (!images || !results))) return LLFE_ERR_INVALID;
    if (n_colors < 0 || n_colors > kMaxColors)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "n_colors=%d outside [1, %d]", n_colors, kMaxColors);
    if (ctx->any_inflight())
        return ctx->fail(LLFE_ERR_INVALID, "llfe_process_images with submitted batches not yet collected");
    ShapePlan pl;
    int bad;
    if (plan_shapes(images, n, preprocessing, pl, &bad)) return bad_plan(ctx, images, bad, preprocessing);
    for (int i = 0; i < n; i++)
        if ((images[i].noise != nullptr) != (images[0].noise != nullptr))
            return ctx->fail(LLFE_ERR_INVALID, "parity noise must be given for every image or for none");
    const bool want_shp = features & LLFE_FEATURE_SHAPES, want_shd = features & LLFE_FEATURE_SHADOWS;
    const uint32_t rest = features & ~(uint32_t)(LLFE_FEATURE_SHAPES | LLFE_FEATURE_SHADOWS);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // The passes run on lane 0's stream, behind the caller's; the host half of a pass (contours
    // on the pool, the records) runs while whatever the caller enqueued on other streams -- the
    // colour pass of LLFE_IMAGES_COLORS_ONE_PASS -- is still on the device.
    Lane &L = ctx->lanes[0];
    HostSlot &H = ctx->slots[0];
    hipStream_t s = L.stream;
    HIPCHK(ctx, hipEventRecord(ctx->start_ev, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamWaitEvent(s, ctx->start_ev, 0));
    for (int i = 0; i < n; i++) {
        std::memset(&results[i], 0, sizeof results[i]);
        results[i].shadow_level = -1;
    }
    int64_t total_shapes = 0;
    for (int k = 0; k < (int)pl.pass.size(); k++) {
        const llfe_shape_pass &p = pl.pass[k];
        // d_bits / d_shadow of the workspace may still be in an earlier D2H
        if (L.mask_reader) HIPCHK(ctx, hipStreamWaitEvent(s, L.mask_reader->mask_done, 0));
        ctx->prof.cur_slot = 0;
        if (int rc = shapes_pass_device(ctx, images, pl, k, want_shp, want_shd, s)) return rc;
        if (int rc = shapes_pass_copy(ctx, p, want_shp, want_shd, s)) return rc;
        HIPCHK(ctx, hipEventSynchronize(H.mask_done));
        if (want_shd) {
            const unsigned long long *sh = H.h_shadow.p;
            for (int j = 0; j < p.count; j++) {
                llfe_image_result &r = results[p.first + j];
                r.shadow_sum = sh[j];
                r.shadow_count = sh[p.count + j];
                r.shadow_level = shadow_level(r.shadow_sum, r.shadow_count);
            }
        }
        if (want_shp)
            host_shapes_from_bits(ctx, H.h_bits.p, p.count, 0, 0, p.first, results, shapes, shape_capacity, total_shapes,
                                  pl.img.data() + p.first);
    }
    HIPCHK(ctx, hipEventRecord(L.stream_done, s));
    HIPCHK(ctx, hipStreamWaitEvent((hipStream_t)stream, L.stream_done, 0));
    ctx->prof.collect();
    if (rest) {
        // fonts (and the colours, when they are not one-pass) by size group; the masks and the sums
        // have left lane 0's workspace, which the groups reuse
        std::vector<llfe_image_result> other((size_t)n);
        int64_t none = 0;
        const int rc = process_images_grouped(ctx, images, n, rest, preprocessing, n_colors, seed, index_base, other.data(),
                                              nullptr, 0, &none, stream);
        if (rc) return rc;
        for (int i = 0; i < n; i++) {
            llfe_image_result r = other[i];
            r.shadow_sum = results[i].shadow_sum;
            r.shadow_count = results[i].shadow_count;
            r.shadow_level = results[i].shadow_level;
            r.shape_offset = results[i].shape_offset;
            r.n_shapes = results[i].n_shapes;
            r.n_contours = results[i].n_contours;
            results[i] = r;
        }
    } else {
        ctx->font_has = false;
        ctx->font_recs.clear();
        ctx->font_owner = LLFE_LAST_CALL;
    }
    if (shapes_needed) *shapes_needed = total_shapes;
    if (want_shp && total_shapes > shape_capacity)
        return ctx->fail(LLFE_ERR_CAPACITY, "shape capacity %lld < %lld", (long long)shape_capacity,
                         (long long)total_shapes);
    return LLFE_OK;
}

extern "C" {

int llfe_shapes_images_layout(const llfe_image_desc *descs, int32_t n, int32_t preprocessing,
                              llfe_shape_image *images, llfe_shape_work *work, int64_t work_capacity,
                              int64_t *n_work, llfe_shape_pass *passes, int32_t pass_capacity, int32_t *n_passes) {
    ShapePlan pl;
    int bad;
    if (int rc = plan_shapes(descs, n, preprocessing, pl, &bad)) return rc;
    if (n_work) *n_work = (int64_t)pl.work.size();
    if (n_passes) *n_passes = (int32_t)pl.pass.size();
    if ((work && work_capacity < (int64_t)pl.work.size()) || (passes && pass_capacity < (int32_t)pl.pass.size()))
        return LLFE_ERR_CAPACITY;
    if (images) std::copy(pl.img.begin(), pl.img.end(), images);
    if (work) std::copy(pl.work.begin(), pl.work.end(), work);
    if (passes) std::copy(pl.pass.begin(), pl.pass.end(), passes);
    return LLFE_OK;
}

int llfe_shape_bits_images(llfe_ctx *ctx, const llfe_image_desc *descs, int32_t n, uint64_t *bits,
                           int64_t bits_capacity_words, llfe_stream stream) {
    if (!ctx || n < 0 || (n > 0 && (!descs || !bits))) return LLFE_ERR_INVALID;
    ShapePlan pl;
    if (int rc = stage_plan(ctx, __func__, descs, n, pl)) return rc;
    const int64_t total = pl.pass.empty() ? 0 : pl.pass.back().first_word + pl.pass.back().words;
    if (bits_capacity_words < total)
        return ctx->fail(LLFE_ERR_CAPACITY, "llfe_shape_bits_images: %lld words < %lld", (long long)bits_capacity_words,
                         (long long)total);
    for (size_t k = 0; k < pl.pass.size(); k++) {
        if (int rc = stage_pass(ctx, descs, pl, (int)k, true, false, (hipStream_t)stream)) return rc;
        std::memcpy(bits + pl.pass[k].first_word, ctx->slots[0].h_bits.p, sizeof(uint64_t) * (size_t)pl.pass[k].words);
    }
    ctx->prof.collect(-2);
    return LLFE_OK;
}

int llfe_shadow_stats_images(llfe_ctx *ctx, const llfe_image_desc *descs, int32_t n, uint64_t *sums,
                             uint64_t *counts, llfe_stream stream) {
    if (!ctx || n < 0 || (n > 0 && (!descs || !sums || !counts))) return LLFE_ERR_INVALID;
    ShapePlan pl;
    if (int rc = stage_plan(ctx, __func__, descs, n, pl)) return rc;
    for (size_t k = 0; k < pl.pass.size(); k++) {
        const llfe_shape_pass &p = pl.pass[k];
        if (int rc = stage_pass(ctx, descs, pl, (int)k, false, true, (hipStream_t)stream)) return rc;
        const unsigned long long *sh = ctx->slots[0].h_shadow.p;
        for (int j = 0; j < p.count; j++) {
            sums[p.first + j] = sh[j];
            counts[p.first + j] = sh[p.count + j];
        }
    }
    ctx->prof.collect(-2);
    return LLFE_OK;
}

int llfe_hysteresis_images(llfe_ctx *ctx, const uint8_t *const *class_maps, const int32_t *heights,
                           const int32_t *widths, int32_t n, int32_t tile_flags, uint64_t *bits_edges,
                           uint64_t *bits_mask, int64_t bits_capacity_words) {
    if (!ctx || n < 0 || (n > 0 && (!class_maps || !heights || !widths)) || (!bits_edges && !bits_mask))
        return LLFE_ERR_INVALID;
    std::vector<llfe_image_desc> descs((size_t)n, llfe_image_desc{});
    for (int i = 0; i < n; i++) {
        descs[i].data = class_maps[i];
        descs[i].height = heights[i];
        descs[i].width = widths[i];
    }
    ShapePlan pl;
    if (int rc = stage_plan(ctx, __func__, descs.data(), n, pl)) return rc;
    if (n == 0) return LLFE_OK;
    if (pl.pass.size() > 1) return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_hysteresis_images: the list does not fit one pass");
    const llfe_shape_pass &p = pl.pass[0];
    if (bits_capacity_words < p.words)
        return ctx->fail(LLFE_ERR_CAPACITY, "llfe_hysteresis_images: %lld words < %lld", (long long)bits_capacity_words,
                         (long long)p.words);
    // the per-tile flag bytes by global tile id: set where the tile holds a candidate
    std::vector<uint8_t> tflag(tile_flags ? (size_t)p.tiles : 0, 0);
    for (int i = 0; i < n; i++) {
        const llfe_shape_image &q = pl.img[i];
        const uint8_t *c = class_maps[i];
        for (int y = 0; y < q.height; y++)
            for (int x = 0; x < q.width; x++) {
                const uint8_t b = c[(size_t)y * q.width + x];
                if (b > 2)
                    return ctx->fail(LLFE_ERR_INVALID, "llfe_hysteresis_images: map %d: class byte %d at (%d, %d) (0, 1 or 2)",
                                     i, b, y, x);
                if (b != 1 && tile_flags) tflag[(size_t)q.first_tile + (y >> 6) * q.tiles_x + (x >> 6)] = 1;
            }
    }
    HIPCHK(ctx, hipDeviceSynchronize());
    Work &W = ctx->lanes[0].W;
    hipStream_t s = ctx->lanes[0].stream;
    HIPCHK(ctx, W.d_cls.ensure((size_t)p.class_bytes));
    PassTables tb;
    if (int rc = pass_tables(ctx, pl, 0, &tb)) return rc;
    if (int rc = upload_tables(ctx, p, s)) return rc;
    for (int i = 0; i < n; i++)
        HIPCHK(ctx, hipMemcpyAsync(W.d_cls.p + pl.img[i].class_offset, class_maps[i], (size_t)pl.img[i].pixels,
                                   hipMemcpyHostToDevice, s));
    if (tile_flags) {
        HIPCHK(ctx, W.d_tflag.ensure(tflag.size()));
        HIPCHK(ctx, hipMemcpyAsync(W.d_tflag.p, tflag.data(), tflag.size(), hipMemcpyHostToDevice, s));
    }
    HystWork wk;
    if (int rc = hyst_work_images(ctx, W, p, tile_flags != 0, &wk)) return rc;
    HIPCHK(ctx, W.d_bits.ensure((size_t)p.words));
    HIPCHK(ctx, launch_hysteresis_dilate_images(W.d_cls.p, tb.dev, wk, W.d_bits.p, s));
    if (bits_edges)
        HIPCHK(ctx, hipMemcpyAsync(bits_edges, W.d_ebits.p, sizeof(uint64_t) * (size_t)p.words, hipMemcpyDeviceToHost, s));
    if (bits_mask)
        HIPCHK(ctx, hipMemcpyAsync(bits_mask, W.d_bits.p, sizeof(uint64_t) * (size_t)p.words, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return LLFE_OK;
}

}  // extern "C"
