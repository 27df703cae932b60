// llfe_process_images[_flags, _routes] and the colours of a batch of images of any sizes in one
// device pass (LLFE_IMAGES_COLORS_ONE_PASS, llfe_color_unique_images): the host planner, the
// staging of the images that cannot be read where they lie, and the pass itself -- the ragged
// k_uq_scatter / k_uq_part over per-image records and a work table (unique.hip), then the
// unchanged k_uq_gather and k-means with the common strides of the pass's largest image.
#include "llfe_ctx.h"

using namespace llfe_host;

namespace {

constexpr int kStepsPerEntry = 2;       // scatter steps one workgroup takes (the uniform launch's share)
constexpr int64_t kMaxEntries = 2048;   // ... stretched so that an image has at most this many entries

struct ColorPlan {
    std::vector<llfe_color_image> img;
    std::vector<llfe_color_work> work;
    std::vector<llfe_color_pass> pass;
    std::vector<int> interp;            // cv2 interpolation of the images the rule resizes
    std::vector<int> max_h, max_w;      // per pass: its largest image
};

inline int64_t align16(int64_t x) { return (x + 15) & ~int64_t(15); }

bool read_in_place(const llfe_image_desc &d, const llfe_color_image &r) {
    return d.on_device && !r.resized && (d.row_stride == 0 || d.row_stride == 3 * (int64_t)d.width);
}

// -> LLFE_OK, or LLFE_ERR_INVALID with *bad = the image (or -1: the arguments)
int plan_colors(const llfe_image_desc *descs, int n, int preprocessing, ColorPlan &pl, int *bad) {
    *bad = -1;
    if (n < 0 || (n > 0 && !descs) || preprocessing < LLFE_PRE_NONE || preprocessing > LLFE_PRE_PERFORMANCE)
        return LLFE_ERR_INVALID;
    pl.img.assign((size_t)n, llfe_color_image{});
    pl.interp.assign((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const llfe_image_desc &d = descs[i];
        *bad = i;
        if (!d.data || !valid_dims(1, d.height, d.width) || (d.row_stride != 0 && d.row_stride < 3 * (int64_t)d.width))
            return LLFE_ERR_INVALID;
        int ow = d.width, oh = d.height, interp = 0;
        const int r = llfe_preprocess_size(d.width, d.height, preprocessing, &ow, &oh, &interp);
        if (r < 0) return LLFE_ERR_INVALID;
        llfe_color_image &q = pl.img[i];
        q.height = r ? oh : d.height;
        q.width = r ? ow : d.width;
        q.resized = r == 1;
        q.pixels = (int64_t)q.height * q.width;
        q.field_pixels = noise_field_pixels(q.pixels);
        q.steps = (int32_t)uq_steps(q.pixels);
        q.stage_offset = -1;
        pl.interp[i] = interp;
    }
    *bad = -1;
    // passes: consecutive images while the count fits the workspace budget of the largest one
    for (int i = 0; i < n;) {
        int count = 0, mh = 0, mw = 0;
        int64_t mp = 0;
        for (; i + count < n; count++) {
            const llfe_color_image &q = pl.img[i + count];
            const bool grows = q.pixels > mp;
            const int cap = std::min(chunk_for(grows ? q.height : mh, grows ? q.width : mw), (int)kMaxKmeansBatch);
            if (count > 0 && count + 1 > cap) break;
            if (grows) mp = q.pixels, mh = q.height, mw = q.width;
        }
        llfe_color_pass p{};
        p.first = i;
        p.count = count;
        p.max_pixels = mp;
        p.tab_steps = (int32_t)uq_steps(mp);
        p.key_stride = (std::max<int64_t>(mp, 1) + 3) & ~int64_t(3);
        p.cube_stride = std::min<int64_t>(p.key_stride, kMaxCubes);
        p.cell_stride = std::min<int64_t>(p.cube_stride, (int64_t)kParts * kCellsPerPart);
        p.work_first = (int32_t)pl.work.size();
        for (int j = i; j < i + count; j++) {
            llfe_color_image &q = pl.img[j];
            q.pass = (int32_t)pl.pass.size();
            if (!read_in_place(descs[j], q)) {
                q.stage_offset = p.stage_bytes;
                p.stage_bytes = align16(p.stage_bytes + q.pixels * 3);
            }
            const int per = (int)std::max<int64_t>(kStepsPerEntry, (q.steps + kMaxEntries - 1) / kMaxEntries);
            for (int st = 0; st < q.steps; st += per) pl.work.push_back(llfe_color_work{j, st, std::min(per, q.steps - st)});
        }
        p.work_count = (int32_t)pl.work.size() - p.work_first;
        pl.pass.push_back(p);
        pl.max_h.push_back(mh);
        pl.max_w.push_back(mw);
        i += count;
    }
    return LLFE_OK;
}

// The colour front of pass k on lane 0's workspace and stream s: stage what cannot be read in
// place, upload the records and the work table, then noise field, scatter, partitions and
// gather.  The pinned table and the staging buffers are free again once s has been waited for.
int color_pass_front(llfe_ctx *ctx, const llfe_image_desc *descs, const ColorPlan &pl, int k, bool with_noise,
                     uint64_t seed, int64_t index_base, bool contiguous_keys, llfe_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    const llfe_color_pass &p = pl.pass[k];
    Work &W = ctx->lanes[0].W;
    HIPCHK(ctx, ctx->d_color_stage.ensure((size_t)std::max<int64_t>(p.stage_bytes, 16)));
    int64_t noise_bytes = 0;
    if (with_noise)
        for (int j = p.first; j < p.first + p.count; j++)
            if (!descs[j].noise_on_device) noise_bytes = align16(noise_bytes + pl.img[j].pixels * 3);
    if (noise_bytes) HIPCHK(ctx, ctx->d_color_noise.ensure((size_t)noise_bytes));
    const size_t rec_bytes = sizeof(UqImgRec) * (size_t)p.count, tab_bytes = rec_bytes + sizeof(UqWork) * (size_t)p.work_count;
    HIPCHK(ctx, ctx->h_uq_tab.ensure(tab_bytes));
    HIPCHK(ctx, ctx->d_uq_tab.ensure(tab_bytes));
    UqImgRec *recs = (UqImgRec *)ctx->h_uq_tab.p;
    UqWork *work = (UqWork *)(ctx->h_uq_tab.p + rec_bytes);
    int64_t noise_off = 0, pixels = 0;
    for (int j = p.first; j < p.first + p.count; j++) {
        const llfe_image_desc &d = descs[j];
        const llfe_color_image &q = pl.img[j];
        const uint8_t *src = d.data;
        if (q.stage_offset >= 0) {
            uint8_t *dst = ctx->d_color_stage.p + q.stage_offset;
            const size_t pitch = d.row_stride ? (size_t)d.row_stride : (size_t)d.width * 3;
            const hipMemcpyKind kind = d.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
            if (!q.resized) {
                HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)d.width * 3, d.data, pitch, (size_t)d.width * 3, d.height, kind, s));
            } else {
                HIPCHK(ctx, ctx->d_rsz_src.ensure((size_t)d.height * d.width * 3));
                HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_rsz_src.p, (size_t)d.width * 3, d.data, pitch, (size_t)d.width * 3,
                                             d.height, kind, s));
                const int rc = llfe_resize_cv(ctx, ctx->d_rsz_src.p, d.height, d.width, 3, dst, q.height, q.width,
                                              pl.interp[j], stream);
                if (rc) return rc;
            }
            src = dst;
        }
        const int8_t *nz = nullptr;
        if (with_noise && d.noise_on_device) {
            nz = d.noise;
        } else if (with_noise) {
            int8_t *dst = ctx->d_color_noise.p + noise_off;
            HIPCHK(ctx, hipMemcpyAsync(dst, d.noise, (size_t)q.pixels * 3, hipMemcpyHostToDevice, s));
            noise_off = align16(noise_off + q.pixels * 3);
            nz = dst;
        }
        recs[j - p.first] = UqImgRec{src, nz, (long long)q.pixels, (long long)q.field_pixels, q.steps, 0};
        pixels += q.pixels;
    }
    for (int e = 0; e < p.work_count; e++) {
        const llfe_color_work &wk = pl.work[(size_t)p.work_first + e];
        work[e] = UqWork{wk.image - p.first, wk.first_step, wk.steps};
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_uq_tab.p, ctx->h_uq_tab.p, tab_bytes, hipMemcpyHostToDevice, s));
    const UqImages rg{(const UqImgRec *)ctx->d_uq_tab.p, (const UqWork *)(ctx->d_uq_tab.p + rec_bytes), p.work_count,
                      p.tab_steps, pixels};
    return color_stage(ctx, W, nullptr, nullptr, with_noise ? recs[0].noise : nullptr, p.count, pl.max_h[k], pl.max_w[k],
                       seed, ImgIndex{index_base + p.first, nullptr}, contiguous_keys, s, &rg);
}

// LLFE_IMAGES_COLORS_ONE_PASS: the device work of colour pass k on stream `stream`, up to the
// D2H of its records into ctx->h_kout
int colors_pass_enqueue(llfe_ctx *ctx, const llfe_image_desc *descs, const ColorPlan &pl, int k, int n_colors,
                        uint64_t seed, int64_t index_base, llfe_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    const llfe_color_pass &p = pl.pass[k];
    const int m = p.count;
    const bool seg = n_colors <= kMaxK;  // (as enqueue_chunk: the keys stay in k_uq_part's layout)
    Work &W = ctx->lanes[0].W;
    ctx->prof.cur_slot = 0;
    int rc = color_pass_front(ctx, descs, pl, k, descs[0].noise != nullptr, seed, index_base, /*contiguous_keys=*/!seg,
                              stream);
    if (rc) return rc;
    ctx->prof.cur_slot = 0;  // (a staging resize tags its own records)
    const KmeansCubes cubes{W.d_cubes.p, p.cube_stride, W.d_ncubes.p, W.d_pmeta.p + (size_t)2 * m * kParts, W.d_cells.p,
                            W.d_ncells.p, p.cell_stride, seg ? W.d_pmeta.p : nullptr, W.d_sups.p, W.d_nsups.p,
                            p.cell_stride, W.d_pmom.p};
    rc = kmeans_stage(ctx, W, seg ? W.d_raw.p : W.d_keys.p, p.key_stride, W.d_nuniq.p, m, n_colors, seed,
                      ImgIndex{index_base + p.first, nullptr}, cubes, s);
    if (rc) return rc;
    HIPCHK(ctx, ctx->h_kout.ensure((size_t)m));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_kout.p, W.d_kout.p, sizeof(KmeansImageOut) * m, hipMemcpyDeviceToHost, s));
    return LLFE_OK;
}

// ... and its host half: wait for it, fill the colour fields of its images' records
int colors_pass_finish(llfe_ctx *ctx, const ColorPlan &pl, int k, int n_colors, llfe_image_result *results,
                       llfe_stream stream) {
    const llfe_color_pass &p = pl.pass[k];
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    const KmeansImageOut *ko = ctx->h_kout.p;
    double kb = 0, ub = 0;
    for (int i = 0; i < p.count; i++) {
        fill_color_result(ko[i], results[p.first + i]);
        kb += (double)ko[i].bytes;
        ub += 4.0 * (double)ko[i].n_unique;
    }
    ctx->prof.collect();
    if (ctx->prof.on) {  // (as finish_chunk charges them)
        ctx->prof.add_bytes("k_kmeans", kb);
        ctx->prof.add_bytes("k_uq_part", ub);
        if (n_colors > kMaxK) ctx->prof.add_bytes("k_uq_gather", ub);
    }
    return LLFE_OK;
}

}  // namespace

extern "C" {

int llfe_colors_images_layout(const llfe_image_desc *descs, int32_t n, int32_t preprocessing,
                              llfe_color_image *images, llfe_color_work *work, int64_t work_capacity,
                              int64_t *n_work, llfe_color_pass *passes, int32_t pass_capacity, int32_t *n_passes) {
    ColorPlan pl;
    int bad;
    if (int rc = plan_colors(descs, n, preprocessing, pl, &bad)) return rc;
    if (n_work) *n_work = (int64_t)pl.work.size();
    if (n_passes) *n_passes = (int32_t)pl.pass.size();
    if ((work && work_capacity < (int64_t)pl.work.size()) || (passes && pass_capacity < (int32_t)pl.pass.size()))
        return LLFE_ERR_CAPACITY;
    if (images) std::copy(pl.img.begin(), pl.img.end(), images);
    if (work) std::copy(pl.work.begin(), pl.work.end(), work);
    if (passes) std::copy(pl.pass.begin(), pl.pass.end(), passes);
    return LLFE_OK;
}

int llfe_process_images_routes(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                               int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                               llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                               int64_t *shapes_needed, llfe_stream stream, uint32_t colors_flags,
                               uint32_t shapes_flags) {
    if ((colors_flags & ~LLFE_IMAGES_COLORS_ONE_PASS) || (shapes_flags & ~LLFE_IMAGES_SHAPES_ONE_PASS))
        return LLFE_ERR_UNSUPPORTED;
    const bool one_pass =
        (colors_flags & LLFE_IMAGES_COLORS_ONE_PASS) && (features & LLFE_FEATURE_COLORS) && ctx && n > 0;
    // shapes and shadows in one pass: not while the context traces contours on the GPU
    // (contours_gpu.hip takes images of one size) -- a call that asks for shapes then goes by
    // size group, with the same results
    const bool shapes_one_pass = (shapes_flags & LLFE_IMAGES_SHAPES_ONE_PASS) &&
                                 (features & (LLFE_FEATURE_SHAPES | LLFE_FEATURE_SHADOWS)) && ctx && n > 0 &&
                                 !(ctx->gpu_contours && (features & LLFE_FEATURE_SHAPES));
    const auto others = shapes_one_pass ? process_images_shapes_one_pass : process_images_grouped;
    if (!one_pass)
        return others(ctx, images, n, features, preprocessing, n_colors, seed, index_base, results, shapes,
                      shape_capacity, shapes_needed, stream);
    // the grouped route's checks, before any work
    if (!images || !results) return LLFE_ERR_INVALID;
    if (n_colors < 0 || n_colors > kMaxColors)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "n_colors=%d outside [1, %d]", n_colors, kMaxColors);
    if (ctx->any_inflight())
        return ctx->fail(LLFE_ERR_INVALID, "llfe_process_images with submitted batches not yet collected");
    ColorPlan pl;
    int bad;
    if (plan_colors(images, n, preprocessing, pl, &bad))
        return bad < 0 ? ctx->fail(LLFE_ERR_INVALID, "preprocessing mode %d", preprocessing)
                       : ctx->fail(LLFE_ERR_INVALID, "image %d: invalid descriptor (%d x %d, stride %lld)", bad,
                                   images[bad].height, images[bad].width, (long long)images[bad].row_stride);
    for (int i = 0; i < n; i++)
        if ((images[i].noise != nullptr) != (images[0].noise != nullptr))
            return ctx->fail(LLFE_ERR_INVALID, "parity noise must be given for every image or for none");
    // The first colour pass goes to the colour stream of lane 0, behind the caller's stream;
    // shapes, shadows and fonts then run beside it on the lanes' own streams -- by size group, or
    // shapes and shadows in one pass of their own (`others`) -- (they share no buffer with it: the
    // pass stages into buffers of its own) and fill every other field of the records; the colour
    // fields follow, and the further passes of a call that does not fit one workspace.
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int K = n_colors ? n_colors : kMaxK;
    llfe_stream cs = (llfe_stream)ctx->lanes[0].col_stream;
    HIPCHK(ctx, hipEventRecord(ctx->start_ev, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamWaitEvent((hipStream_t)cs, ctx->start_ev, 0));
    if (int rc = colors_pass_enqueue(ctx, images, pl, 0, K, seed, index_base, cs)) return rc;
    const uint32_t rest = features & ~(uint32_t)LLFE_FEATURE_COLORS;
    int rc_rest = LLFE_OK;
    if (rest) {
        rc_rest = others(ctx, images, n, rest, preprocessing, n_colors, seed, index_base, results, shapes, shape_capacity,
                         shapes_needed, stream);
        if (rc_rest && rc_rest != LLFE_ERR_CAPACITY) {  // (short capacity: the results are valid)
            (void)hipStreamSynchronize((hipStream_t)cs);
            return rc_rest;
        }
    } else {
        for (int i = 0; i < n; i++) {
            std::memset(&results[i], 0, sizeof results[i]);
            results[i].shadow_level = -1;
        }
        ctx->font_has = false;
        ctx->font_recs.clear();
        ctx->font_owner = LLFE_LAST_CALL;
        if (shapes_needed) *shapes_needed = 0;
    }
    const std::string err_rest = ctx->err;
    for (int k = 0; k < (int)pl.pass.size(); k++) {
        if (k > 0)
            if (int rc = colors_pass_enqueue(ctx, images, pl, k, K, seed, index_base, cs)) return rc;
        if (int rc = colors_pass_finish(ctx, pl, k, K, results, cs)) return rc;
    }
    if (rc_rest) ctx->err = err_rest;
    return rc_rest;
}

int llfe_process_images_flags(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                              int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                              llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                              int64_t *shapes_needed, llfe_stream stream, uint32_t flags) {
    if (flags & ~LLFE_IMAGES_COLORS_ONE_PASS) return LLFE_ERR_UNSUPPORTED;
    return llfe_process_images_routes(ctx, images, n, features, preprocessing, n_colors, seed, index_base, results, shapes,
                                      shape_capacity, shapes_needed, stream, flags, 0);
}

int llfe_process_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                        int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                        llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                        int64_t *shapes_needed, llfe_stream stream) {
    return llfe_process_images_flags(ctx, images, n, features, preprocessing, n_colors, seed, index_base, results, shapes,
                                     shape_capacity, shapes_needed, stream, 0);
}

int llfe_color_unique_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint64_t seed,
                             int64_t index_base, uint32_t *keys, int64_t key_stride, int64_t *n_unique,
                             llfe_stream stream) {
    if (!ctx || n < 0 || (n > 0 && (!images || !keys || !n_unique))) return LLFE_ERR_INVALID;
    if (int rc_ = stage_enter(ctx, __func__)) return rc_;
    ColorPlan pl;
    int bad;
    if (plan_colors(images, n, LLFE_PRE_NONE, pl, &bad)) return ctx->fail(LLFE_ERR_INVALID, "image %d: invalid descriptor", bad);
    for (int i = 0; i < n; i++) {
        if ((images[i].noise != nullptr) != (images[0].noise != nullptr))
            return ctx->fail(LLFE_ERR_INVALID, "parity noise must be given for every image or for none");
        if (pl.img[i].pixels > key_stride)
            return ctx->fail(LLFE_ERR_INVALID, "image %d: %lld pixels exceed key_stride %lld", i, (long long)pl.img[i].pixels,
                             (long long)key_stride);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    Work &W = ctx->lanes[0].W;
    for (size_t k = 0; k < pl.pass.size(); k++) {
        const llfe_color_pass &p = pl.pass[k];
        const int rc = color_pass_front(ctx, images, pl, (int)k, images[0].noise != nullptr, seed, index_base,
                                        /*contiguous_keys=*/true, stream);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(keys + (size_t)p.first * key_stride, sizeof(uint32_t) * key_stride, W.d_keys.p,
                                     sizeof(uint32_t) * p.key_stride, sizeof(uint32_t) * p.max_pixels, p.count,
                                     hipMemcpyDeviceToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(n_unique + p.first, W.d_nuniq.p, sizeof(int64_t) * p.count, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    ctx->prof.collect(-2);
    return LLFE_OK;
}

}  // extern "C"
