// C ABI of libllfe.so (include/llfe.h): cv2.resize of a batch of images of any sizes in one
// device pass -- validate_and_preprocess_image's resize over a batch (llfe_preprocess_images) and
// its stage entry with explicit sizes (llfe_resize_cv_images); kernels in cvresize_images.hip.
#include <chrono>
#include <map>
#include <tuple>

#include "llfe_ctx.h"

using namespace llfe_host;

namespace {

// The staging workspace is bounded: host sources go through it in chunks of images on the one
// stream (a chunk's kernels are ordered before the next chunk's copies).  256 MiB is seven
// 12 MP sources.
constexpr int64_t kCvStageBudget = (int64_t)256 << 20;
constexpr int kKinds = 4;  // CvResizePlan::Kind

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

bool valid_image_desc(const llfe_image_desc &d) {
    return d.data && valid_dims(1, d.height, d.width) && (d.row_stride == 0 || d.row_stride >= 3 * (int64_t)d.width);
}

// what one image asks for
struct Req {
    int32_t oh = 0, ow = 0, interp = 0;
    bool resized = false;
};

// the rule of validate_and_preprocess_image per image; -> LLFE_OK or LLFE_ERR_INVALID with *bad
// the first image the rule cannot size (a side of 0: cv2.resize raises there)
int rule_reqs(const llfe_image_desc *images, int n, int32_t mode, std::vector<Req> &reqs, int *bad) {
    reqs.assign((size_t)n, Req{});
    for (int i = 0; i < n; i++) {
        int32_t ow = 0, oh = 0, interp = 0;
        const int rc = llfe_preprocess_size(images[i].width, images[i].height, mode, &ow, &oh, &interp);
        *bad = i;
        if (rc < 0) return LLFE_ERR_INVALID;
        Req &q = reqs[i];
        if (rc == 0) {
            q.oh = images[i].height, q.ow = images[i].width;
            continue;
        }
        if (oh <= 0 || ow <= 0) return LLFE_ERR_INVALID;
        q.oh = oh, q.ow = ow, q.interp = interp, q.resized = true;
    }
    return LLFE_OK;
}

// explicit (out_h, out_w, interpolation) triples
int sizes_reqs(const llfe_image_desc *images, int n, const int32_t *sizes3, std::vector<Req> &reqs, int *bad) {
    reqs.assign((size_t)n, Req{});
    for (int i = 0; i < n; i++) {
        const int32_t oh = sizes3[3 * i], ow = sizes3[3 * i + 1], interp = sizes3[3 * i + 2];
        *bad = i;
        if (interp == LLFE_CV_INTER_CUBIC) return LLFE_ERR_UNSUPPORTED;
        if (interp != LLFE_CV_INTER_LINEAR && interp != LLFE_CV_INTER_AREA && interp != LLFE_CV_INTER_LANCZOS4)
            return LLFE_ERR_INVALID;
        if (!valid_dims(1, oh, ow)) return LLFE_ERR_INVALID;
        Req &q = reqs[i];
        q.oh = oh, q.ow = ow;
        q.resized = oh != images[i].height || ow != images[i].width;
        q.interp = q.resized ? interp : 0;
    }
    return LLFE_OK;
}

int64_t layout(const llfe_image_desc *images, int n, const std::vector<Req> &reqs, llfe_resize_out *outs) {
    int64_t end = 0;
    for (int i = 0; i < n; i++) {
        outs[i].offset = align16(end);
        outs[i].height = reqs[i].oh, outs[i].width = reqs[i].ow;
        outs[i].interpolation = reqs[i].interp, outs[i].resized = reqs[i].resized ? 1 : 0;
        end = outs[i].offset + (int64_t)reqs[i].oh * reqs[i].ow * 3;
    }
    return end;
}

bool valid_args(const llfe_image_desc *images, int n, const void *outs, const int64_t *dst_bytes) {
    if (n < 0 || !dst_bytes || (n > 0 && (!images || !outs))) return false;
    for (int i = 0; i < n; i++)
        if (!valid_image_desc(images[i])) return false;
    return true;
}

// the plan of one distinct (h, w, oh, ow, interpolation) of a call, with what the kernels need
struct ImgPlan {
    int h = 0, w = 0, oh = 0, ow = 0, interp = 0;
    llfe::CvResizePlan p;
    int tile_h = llfe::kCvTileH, arm = llfe::kCvArmLds;
    int64_t tab = 0;  // offset of the plan's tables in the call's int32 table
    const char *err = nullptr;
};

// one area table as area_tab lays it out: [dsize + 1] starts, then (si, weight) pairs.  Checks
// what the kernels rely on: starts ascend from 0 to the pair count, every output has a pair,
// every si is a multiple of `step` in [0, max_si] and the sis ascend.
bool area_tab_ok(const int32_t *t, int64_t len, int dsize, int max_si, int step) {
    if (len < dsize + 1 || t[0] != 0) return false;
    const int64_t np = t[dsize];
    if (np < dsize || len != dsize + 1 + 2 * np) return false;
    for (int d = 0; d < dsize; d++)
        if (t[d + 1] <= t[d]) return false;
    const int32_t *p = t + dsize + 1;
    int prev = 0;
    for (int64_t k = 0; k < np; k++) {
        const int si = p[2 * k];
        if (si < prev || si > max_si || si % step) return false;
        prev = si;
    }
    return true;
}

// Builds the plan and checks everything the kernels index with against the sizes and the
// kernels' compile-time budgets: nothing is launched on a plan that has not passed here.
void cv_images_plan_check(ImgPlan &P) {
    using namespace llfe;
    if (cv_resize_plan(P.h, P.w, 3, P.oh, P.ow, P.interp, P.p) != 0) {
        P.err = "no resize plan";
        return;
    }
    CvResizePlan &p = P.p;
    const auto global_arm = [&] { P.arm = kCvArmGlobal, P.tile_h = kCvGenericTileH; };
    switch (p.kind) {
    case CvResizePlan::COPY: break;
    case CvResizePlan::AREA_FAST: {
        if (p.fx < 1 || p.fy < 1 || (int64_t)p.fx * P.ow > (int64_t)P.w + p.fx || (int64_t)p.fy * P.oh > (int64_t)P.h + p.fy) {
            P.err = "integer factors outside the source";
            return;
        }
        const int64_t pitch = ((int64_t)kCvTileW * p.fx * 3 + 6) & ~(int64_t)3;
        int th = kCvTileH;
        while (th >= 1 && (int64_t)th * p.fy * pitch > kCvFastStageBytes) th /= 2;
        if (th >= 1) P.tile_h = th;
        else global_arm();
        break;
    }
    case CvResizePlan::AREA: {
        const int32_t *xt = p.tab.data(), *yt = xt + p.ytab_off;
        if (p.ytab_off <= 0 || p.ytab_off >= (int64_t)p.tab.size() ||
            !area_tab_ok(xt, p.ytab_off, P.ow, (P.w - 1) * 3, 3) ||
            !area_tab_ok(yt, (int64_t)p.tab.size() - p.ytab_off, P.oh, P.h - 1, 1)) {
            P.err = "area tables outside the source";
            return;
        }
        const int32_t *xp = xt + P.ow + 1, *yp = yt + P.oh + 1;
        bool x_fits = true;
        for (int x0 = 0; x0 < P.ow && x_fits; x0 += kCvTileW) {
            const int x1 = std::min(P.ow, x0 + kCvTileW);
            const int k0 = xt[x0], nk = xt[x1] - k0;
            const int64_t span = (int64_t)xp[2 * (k0 + nk - 1)] + 3 - xp[2 * k0];
            x_fits = nk <= kCvMaxPairs && ((span + 6) & ~(int64_t)3) <= kCvStageBytes;
        }
        int th = x_fits ? kCvTileH : 0;
        for (; th >= 1; th /= 2) {
            bool fits = true;
            for (int y0 = 0; y0 < P.oh && fits; y0 += th) {
                const int y1 = std::min(P.oh, y0 + th);
                const int k0 = yt[y0], nk = yt[y1] - k0;
                fits = nk <= kCvMaxYPairs && yp[2 * (k0 + nk - 1)] - yp[2 * k0] + 1 <= kCvLdsRows;
            }
            if (fits) break;
        }
        if (th >= 1) P.tile_h = th;
        else global_arm();
        break;
    }
    case CvResizePlan::GENERIC:
        // (the kernel clamps every source index it forms; the tables are indexed by output pixel)
        if ((p.ks != 2 && p.ks != 8) || p.ytab_off != (int64_t)P.ow * (1 + p.ks) ||
            (int64_t)p.tab.size() != p.ytab_off + (int64_t)P.oh * (1 + p.ks)) {
            P.err = "generic tables of another size than the kernel reads";
            return;
        }
        P.tile_h = kCvGenericTileH;
        break;
    }
}

int resize_images(llfe_ctx *ctx, const char *fn, const llfe_image_desc *images, int n, const std::vector<Req> &reqs,
                  uint8_t *dst, const llfe_resize_out *outs, hipStream_t s) {
    using namespace llfe;
    const auto t_plan = std::chrono::steady_clock::now();
    // one plan per distinct (h, w, out size, interpolation), built on the pool
    std::vector<ImgPlan> plans;
    std::vector<int> plan_of((size_t)n);
    {
        std::map<std::tuple<int, int, int, int, int>, int> seen;
        for (int i = 0; i < n; i++) {
            // (an image that keeps its size is a copy whatever the interpolation)
            const int interp = reqs[i].resized ? reqs[i].interp : kCvInterArea;
            const auto key = std::make_tuple(images[i].height, images[i].width, reqs[i].oh, reqs[i].ow, interp);
            auto f = seen.find(key);
            if (f == seen.end()) {
                f = seen.emplace(key, (int)plans.size()).first;
                plans.emplace_back();
                ImgPlan &P = plans.back();
                P.h = images[i].height, P.w = images[i].width, P.oh = reqs[i].oh, P.ow = reqs[i].ow, P.interp = interp;
            }
            plan_of[i] = f->second;
        }
    }
    auto build = [&](int p, int) { cv_images_plan_check(plans[p]); };
    if (ctx->pool)
        ctx->pool->parallel_for((int)plans.size(), build);
    else
        for (size_t p = 0; p < plans.size(); p++) build((int)p, 0);
    int64_t tab_n = 0;
    for (ImgPlan &P : plans) {
        if (P.err)
            return ctx->fail(LLFE_ERR_UNSUPPORTED, "%s: %d x %d -> %d x %d: %s", fn, P.h, P.w, P.oh, P.ow, P.err);
        P.tab = tab_n;
        tab_n += (int64_t)P.p.tab.size();
    }
    // per image: workspace bytes (a staged host source) and work entries of its kind
    struct Item {
        int64_t stage = 0, ws = 0, n_work = 0;
        bool direct = false;  // a host image that keeps its size: one 2-D copy into dst
    };
    std::vector<Item> it((size_t)n);
    int64_t total[kKinds] = {0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
        const ImgPlan &P = plans[plan_of[i]];
        Item &q = it[i];
        if (P.p.kind == CvResizePlan::COPY && !images[i].on_device) {
            q.direct = true;
            continue;
        }
        if (!images[i].on_device) q.stage = align16((int64_t)P.h * P.w * 3);
        q.n_work = (int64_t)((P.ow + kCvTileW - 1) / kCvTileW) * ((P.oh + P.tile_h - 1) / P.tile_h);
        total[P.p.kind] += q.n_work;
    }
    int64_t all_work = 0;
    for (int k = 0; k < kKinds; k++) all_work += total[k];
    if (all_work >= (1LL << 31) || tab_n >= (1LL << 31))
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "%s: the batch needs too many tiles for one call", fn);
    // chunks of consecutive images whose staged sources fit the budget (one image always fits)
    int64_t budget = kCvStageBudget;
    if (const char *e = getenv("LLFE_RESIZE_STAGE_BYTES"); e && atoll(e) > 0) budget = atoll(e);  // (tests: many chunks)
    struct Chunk {
        int i0, i1;
        int64_t w0[kKinds], w1[kKinds];  // its entries of the work tables
    };
    std::vector<Chunk> chunks;
    int64_t ws_bytes = 0;
    {
        int64_t used = 0, at[kKinds] = {0, 0, 0, 0};
        Chunk c{};
        for (int i = 0; i < n; i++) {
            if (i > c.i0 && it[i].stage > 0 && used + it[i].stage > budget) {
                c.i1 = i;
                for (int k = 0; k < kKinds; k++) c.w1[k] = at[k];
                chunks.push_back(c);
                c.i0 = i;
                for (int k = 0; k < kKinds; k++) c.w0[k] = at[k];
                used = 0;
            }
            it[i].ws = used;
            used += it[i].stage;
            ws_bytes = std::max(ws_bytes, used);
            at[plans[plan_of[i]].p.kind] += it[i].n_work;
        }
        c.i1 = n;
        for (int k = 0; k < kKinds; k++) c.w1[k] = at[k];
        chunks.push_back(c);
    }
    HIPCHK(ctx, ctx->d_cvimg_ws.ensure((size_t)std::max<int64_t>(ws_bytes, 16)));
    // one pinned block: [int32 table | records | work tables by kind], one upload
    int64_t o_work[kKinds];
    const int64_t o_rec = align16(tab_n * 4);
    int64_t blk = o_rec + align16((int64_t)n * sizeof(CvImgRec));
    for (int k = 0; k < kKinds; k++) {
        o_work[k] = blk;
        blk += align16(total[k] * (int64_t)sizeof(CvImgWork));
    }
    HIPCHK(ctx, ctx->h_cvimg_tab.ensure((size_t)blk));
    HIPCHK(ctx, ctx->d_cvimg_tab.ensure((size_t)blk));
    uint8_t *hb = ctx->h_cvimg_tab.p, *db = ctx->d_cvimg_tab.p;
    int32_t *tab = (int32_t *)hb;
    for (const ImgPlan &P : plans)
        if (!P.p.tab.empty()) std::memcpy(tab + P.tab, P.p.tab.data(), P.p.tab.size() * sizeof(int32_t));
    CvImgRec *recs = (CvImgRec *)(hb + o_rec);
    CvImgWork *wp[kKinds];
    for (int k = 0; k < kKinds; k++) wp[k] = (CvImgWork *)(hb + o_work[k]);
    double bytes[kKinds] = {0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
        const ImgPlan &P = plans[plan_of[i]];
        const llfe_image_desc &d = images[i];
        const Item &q = it[i];
        CvImgRec &r = recs[i];
        std::memset(&r, 0, sizeof r);
        if (q.direct) continue;
        r.src = d.on_device ? d.data : ctx->d_cvimg_ws.p + q.ws;
        r.src_stride = d.on_device && d.row_stride ? d.row_stride : (int64_t)d.width * 3;
        r.dst = dst + outs[i].offset;
        r.h = P.h, r.w = P.w, r.oh = P.oh, r.ow = P.ow;
        r.kind = P.p.kind, r.fx = P.p.fx, r.fy = P.p.fy;
        r.ks = P.p.ks, r.xmax = P.p.xmax, r.x_vec = P.p.x_vec;
        r.xt = (int32_t)P.tab, r.yt = (int32_t)(P.tab + P.p.ytab_off);
        r.tile_h = P.tile_h, r.tiles_x = (P.ow + kCvTileW - 1) / kCvTileW, r.arm = P.arm;
        for (int64_t t = 0; t < q.n_work; t++) *wp[r.kind]++ = CvImgWork{i, (int32_t)t};
        bytes[r.kind] += (double)P.h * P.w * 3 + (double)P.oh * P.ow * 3;
    }
    if (ctx->prof.on) {  // the host plan beside the kernels in llfe_kernel_stats
        Profiler::Stat &st = ctx->prof.stats[ctx->prof.kid("cv_images_plan_host")];
        st.launches++;
        st.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_plan).count();
    }
    HIPCHK(ctx, hipMemcpyAsync(db, hb, (size_t)blk, hipMemcpyHostToDevice, s));
    const CvImgRec *d_recs = (const CvImgRec *)(db + o_rec);
    static const char *const names[kKinds] = {"k_cv_images_copy", "k_cv_images_area_fast", "k_cv_images_area",
                                              "k_cv_images_generic"};
    static_assert(CvResizePlan::COPY == 0 && CvResizePlan::AREA_FAST == 1 && CvResizePlan::AREA == 2 &&
                      CvResizePlan::GENERIC == 3,
                  "names follow CvResizePlan::Kind");
    for (const Chunk &c : chunks) {
        StageSlotScope tag(ctx->prof);
        for (int i = c.i0; i < c.i1; i++) {
            const llfe_image_desc &d = images[i];
            if (d.on_device) continue;
            const size_t pitch = d.row_stride ? (size_t)d.row_stride : (size_t)d.width * 3, row = (size_t)d.width * 3;
            uint8_t *to = it[i].direct ? dst + outs[i].offset : ctx->d_cvimg_ws.p + it[i].ws;
            HIPCHK(ctx, hipMemcpy2DAsync(to, row, d.data, pitch, row, d.height, hipMemcpyHostToDevice, s));
        }
        for (int k = 0; k < kKinds; k++) {
            const int64_t nw = c.w1[k] - c.w0[k];
            if (nw <= 0) continue;
            TIMED(ctx, s, names[k], bytes[k] / (double)total[k] * (double)nw,
                  launch_cv_images(k, d_recs, (const CvImgWork *)(db + o_work[k]) + c.w0[k], (int)nw,
                                   (const int32_t *)db, s));
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(s));  // the pinned block and the workspace are free again
    ctx->prof.collect(Profiler::kStageSlot);
    return LLFE_OK;
}

// the checks every entry shares, then the call
int run(llfe_ctx *ctx, const char *fn, const llfe_image_desc *images, int32_t n, int rc_reqs, int bad,
        const std::vector<Req> &reqs, uint8_t *dst, int64_t dst_capacity, llfe_resize_out *outs, llfe_stream stream) {
    if (rc_reqs != LLFE_OK)
        return ctx->fail(rc_reqs, "%s: image %d (%d x %d): %s", fn, bad, images[bad].height, images[bad].width,
                         rc_reqs == LLFE_ERR_UNSUPPORTED ? "INTER_CUBIC is not taken here (llfe_resize_cv)"
                                                         : "no valid result size or interpolation");
    if ((n > 0 && !dst) || dst_capacity < 0) return ctx->fail(LLFE_ERR_INVALID, "%s: bad destination", fn);
    const int64_t total = layout(images, n, reqs, outs);
    if (n == 0) return LLFE_OK;
    if (total > dst_capacity)
        return ctx->fail(LLFE_ERR_CAPACITY, "%s: dst holds %lld bytes, the layout needs %lld", fn,
                         (long long)dst_capacity, (long long)total);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return resize_images(ctx, fn, images, n, reqs, dst, outs, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int llfe_preprocess_images_layout(const llfe_image_desc *images, int32_t n, int32_t preprocessing,
                                  llfe_resize_out *outs, int64_t *dst_bytes) {
    if (!valid_args(images, n, outs, dst_bytes)) return LLFE_ERR_INVALID;
    if (preprocessing < LLFE_PRE_NONE || preprocessing > LLFE_PRE_PERFORMANCE) return LLFE_ERR_INVALID;
    std::vector<Req> reqs;
    int bad = 0;
    if (rule_reqs(images, n, preprocessing, reqs, &bad) != LLFE_OK) return LLFE_ERR_INVALID;
    *dst_bytes = layout(images, n, reqs, outs);
    return LLFE_OK;
}

// validate_and_preprocess_image's resize (utils.py:118-143) of n images of any sizes in one
// device pass: one plan per distinct (size, result size, interpolation), one upload of every
// table, one launch per plan kind and staging chunk (cvresize_images.hip), one synchronisation
// at the end
int llfe_preprocess_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, int32_t preprocessing,
                           uint8_t *dst, int64_t dst_capacity, llfe_resize_out *outs, llfe_stream stream) {
    static const char fn[] = "llfe_preprocess_images";
    if (!ctx) return LLFE_ERR_INVALID;
    int64_t total = 0;
    if (!valid_args(images, n, outs, &total))
        return ctx->fail(LLFE_ERR_INVALID, "%s: bad arguments or an invalid image descriptor", fn);
    if (preprocessing < LLFE_PRE_NONE || preprocessing > LLFE_PRE_PERFORMANCE)
        return ctx->fail(LLFE_ERR_INVALID, "%s: preprocessing mode %d", fn, preprocessing);
    std::vector<Req> reqs;
    int bad = 0;
    const int rc = rule_reqs(images, n, preprocessing, reqs, &bad);
    return run(ctx, fn, images, n, rc, bad, reqs, dst, dst_capacity, outs, stream);
}

int llfe_resize_cv_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, const int32_t *sizes3,
                          uint8_t *dst, int64_t dst_capacity, llfe_resize_out *outs, llfe_stream stream) {
    static const char fn[] = "llfe_resize_cv_images";
    if (!ctx) return LLFE_ERR_INVALID;
    int64_t total = 0;
    if (!valid_args(images, n, outs, &total) || (n > 0 && !sizes3))
        return ctx->fail(LLFE_ERR_INVALID, "%s: bad arguments or an invalid image descriptor", fn);
    std::vector<Req> reqs;
    int bad = 0;
    const int rc = sizes_reqs(images, n, sizes3, reqs, &bad);
    return run(ctx, fn, images, n, rc, bad, reqs, dst, dst_capacity, outs, stream);
}

int llfe_resize_cv_images_tiling(int32_t *tile_w, int32_t *tile_h, int32_t *lds_rows) {
    if (!tile_w || !tile_h || !lds_rows) return LLFE_ERR_INVALID;
    *tile_w = llfe::kCvTileW, *tile_h = llfe::kCvTileH, *lds_rows = llfe::kCvLdsRows;
    return LLFE_OK;
}

}  // extern "C"
