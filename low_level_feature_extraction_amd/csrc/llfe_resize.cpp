// C ABI of libllfe.so (include/llfe.h): Pillow LANCZOS resize / thumbnail / reduce, cv2.resize
// and the text binary.
#include <chrono>
#include <cmath>
#include <map>

#include "llfe_ctx.h"

using namespace llfe_host;

namespace {

// Pillow precompute_coeffs (LANCZOS, support 3) -> 22-bit fixed point
int pil_coeffs(int in_size, double in0, double in1, int out_size, std::vector<int32_t> &bounds,
               std::vector<int32_t> &kk) {
    double scale = (double)((float)in1 - (float)in0) / out_size;  // Pillow subtracts its float arguments as floats
    double filterscale = scale < 1.0 ? 1.0 : scale;
    double support = 3.0 * filterscale;
    int ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> k(ksize);
    auto sinc = [](double x) {
        if (x == 0.0) return 1.0;
        x = x * M_PI;
        return std::sin(x) / x;
    };
    auto lanczos = [&](double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; };
    for (int xx = 0; xx < out_size; xx++) {
        double center = in0 + (xx + 0.5) * scale;
        double ww = 0.0, ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        int x = 0;
        for (; x < xmax; x++) {
            double wv = lanczos((x + xmin - center + 0.5) * ss);
            k[x] = wv;
            ww += wv;
        }
        for (x = 0; x < xmax; x++)
            if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; x++) k[x] = 0;
        for (x = 0; x < ksize; x++) {
            double v = k[x] * (1 << 22);
            kk[(size_t)xx * ksize + x] = v < 0 ? (int32_t)(-0.5 + v) : (int32_t)(0.5 + v);
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

// Host plan of Image.resize(size, LANCZOS, box) of an h x w image: which passes run, their
// coefficient tables and the source rows the horizontal pass has to produce.  Shared by the
// same-size entry points and llfe_thumbnail_pil_images.
struct LanczosPlan {
    int h = 0, w = 0, oh = 0, ow = 0;
    bool need_h = false, need_v = false;
    int ksh = 0, ksv = 0;
    int yfirst = 0, ylast = 0;  // source rows [yfirst, ylast) feed the vertical pass
    // bounds (xmin, count per output index) and 22-bit coefficients; with need_h, bv's xmin
    // is relative to yfirst (the horizontal pass starts its output there)
    std::vector<int32_t> bh, kh, bv, kv;
};

void lanczos_plan(int32_t h, int32_t w, int32_t out_h, int32_t out_w, const double *box, LanczosPlan &p) {
    // Pillow hands the box of Image.resize to its C code as four 32-bit floats: w / 3 arrives there
    // rounded to float32, and the coefficients follow from that value
    auto f32 = [](double v) { return (double)(float)v; };
    double bx0 = box ? f32(box[0]) : 0, by0 = box ? f32(box[1]) : 0, bx1 = box ? f32(box[2]) : w,
           by1 = box ? f32(box[3]) : h;
    p.h = h, p.w = w, p.oh = out_h, p.ow = out_w;
    p.need_h = out_w != w || bx0 != 0 || bx1 != out_w;
    p.need_v = out_h != h || by0 != 0 || by1 != out_h;
    p.ksh = pil_coeffs(w, bx0, bx1, out_w, p.bh, p.kh);
    p.ksv = pil_coeffs(h, by0, by1, out_h, p.bv, p.kv);
    p.yfirst = p.bv[0], p.ylast = p.bv[2 * out_h - 2] + p.bv[2 * out_h - 1];
    if (p.need_h)
        for (int i = 0; i < out_h; i++) p.bv[2 * i] -= p.yfirst;
}

// Image.thumbnail((max_w, max_h), LANCZOS) of an h x w image: the size rule, the factors of
// reducing_gap = 2.0's reduce() pre-pass and the box it leaves for the resize
struct ThumbGeom {
    int ow = 0, oh = 0;
    bool resized = false;
    int fx = 1, fy = 1;
    int rw = 0, rh = 0;  // size after the pre-pass (the source's own without one)
    double box[4] = {0, 0, 0, 0};
    bool reduced() const { return fx > 1 || fy > 1; }
};

int thumb_geometry(int32_t h, int32_t w, int32_t max_w, int32_t max_h, ThumbGeom &g) {
    int32_t ow, oh;
    int rc = llfe_thumbnail_size(w, h, max_w, max_h, &ow, &oh);
    if (rc < 0) return rc;
    g.ow = ow, g.oh = oh, g.resized = rc == 1, g.rw = w, g.rh = h;
    if (!g.resized) return rc;
    // Image.resize(size, LANCZOS, box=None, reducing_gap=2.0)
    const double gap = 2.0;
    g.fx = std::max(1, (int)((double)w / ow / gap));
    g.fy = std::max(1, (int)((double)h / oh / gap));
    if (g.reduced()) {
        // _get_safe_box of the full image is the full image itself
        g.rw = (w + g.fx - 1) / g.fx, g.rh = (h + g.fy - 1) / g.fy;
        g.box[2] = (double)w / g.fx, g.box[3] = (double)h / g.fy;
    }
    return rc;
}

// Image.resize(size, LANCZOS, box) of n same-size packed device images
int resize_lanczos_n(llfe_ctx *ctx, const uint8_t *src, int n, int32_t h, int32_t w, int32_t ch, uint8_t *dst,
                     int32_t out_h, int32_t out_w, const double *box, hipStream_t s) {
    LanczosPlan p;
    lanczos_plan(h, w, out_h, out_w, box, p);
    const bool need_h = p.need_h, need_v = p.need_v;
    const int ksh = p.ksh, ksv = p.ksv, yfirst = p.yfirst, ylast = p.ylast;
    // coefficient block: [bh | kh | bv | kv]
    size_t nb = p.bh.size() + p.kh.size() + p.bv.size() + p.kv.size();
    HIPCHK(ctx, ctx->d_coef.ensure(nb));
    std::vector<int32_t> all;
    all.reserve(nb);
    all.insert(all.end(), p.bh.begin(), p.bh.end());
    all.insert(all.end(), p.kh.begin(), p.kh.end());
    all.insert(all.end(), p.bv.begin(), p.bv.end());
    all.insert(all.end(), p.kv.begin(), p.kv.end());
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef.p, all.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int32_t *dbh = ctx->d_coef.p, *dkh = dbh + p.bh.size(), *dbv = dkh + p.kh.size(), *dkv = dbv + p.bv.size();
    const long long in_img = (long long)h * w * ch, out_img = (long long)out_h * out_w * ch;
    StageSlotScope tag(ctx->prof);
    if (!need_h && !need_v) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)n * in_img, hipMemcpyDeviceToDevice, s));
    } else if (need_h && !need_v) {
        TIMED(ctx, s, "k_resize_h", (double)n * (in_img + out_img),
              launch_resize_h(src, h, w, ch, yfirst, ylast - yfirst, dst, out_w, dbh, dkh, ksh, s, n, in_img, out_img));
    } else if (!need_h) {
        TIMED(ctx, s, "k_resize_v", (double)n * (in_img + out_img),
              launch_resize_v(src, w, ch, dst, out_h, dbv, dkv, ksv, s, n, in_img, out_img));
    } else {
        const int rows = ylast - yfirst;
        const long long tmp_img = (long long)rows * out_w * ch;
        HIPCHK(ctx, ctx->d_rsz_tmp.ensure((size_t)n * tmp_img));
        TIMED(ctx, s, "k_resize_h", (double)n * (in_img + tmp_img),
              launch_resize_h(src, h, w, ch, yfirst, rows, ctx->d_rsz_tmp.p, out_w, dbh, dkh, ksh, s, n, in_img, tmp_img));
        TIMED(ctx, s, "k_resize_v", (double)n * (tmp_img + out_img),
              launch_resize_v(ctx->d_rsz_tmp.p, out_w, ch, dst, out_h, dbv, dkv, ksv, s, n, tmp_img, out_img));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));  // host coefficient vectors die here
    ctx->prof.collect(Profiler::kStageSlot);
    return LLFE_OK;
}

// thumbnail((max_w, max_h), LANCZOS) incl. the reducing_gap=2.0 reduce() pre-pass, n images
int thumbnail_n(llfe_ctx *ctx, const uint8_t *src, int n, int32_t h, int32_t w, int32_t ch, int32_t max_w,
                int32_t max_h, uint8_t *dst, int64_t dst_capacity, int32_t *out_h, int32_t *out_w, hipStream_t s) {
    ThumbGeom g;
    int rc = thumb_geometry(h, w, max_w, max_h, g);
    if (rc < 0) return ctx->fail(rc, "invalid thumbnail geometry");
    const int32_t ow = g.ow, oh = g.oh;
    if ((int64_t)n * ow * oh * ch > dst_capacity) return ctx->fail(LLFE_ERR_CAPACITY, "thumbnail dst too small");
    *out_w = ow;
    *out_h = oh;
    if (rc == 0) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)n * h * w * ch, hipMemcpyDeviceToDevice, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return LLFE_OK;
    }
    if (g.reduced()) {
        const long long red_img = (long long)g.rw * g.rh * ch;
        HIPCHK(ctx, ctx->d_rsz_src.ensure((size_t)n * red_img));
        {
            StageSlotScope tag(ctx->prof);
            TIMED(ctx, s, "k_reduce", (double)n * ((double)h * w * ch + red_img),
                  launch_reduce(src, w, ch, 0, 0, w, h, g.fx, g.fy, ctx->d_rsz_src.p, g.rw, g.rh, s, n,
                                (long long)h * w * ch, red_img));
        }
        return resize_lanczos_n(ctx, ctx->d_rsz_src.p, n, g.rh, g.rw, ch, dst, oh, ow, g.box, s);
    }
    return resize_lanczos_n(ctx, src, n, h, w, ch, dst, oh, ow, nullptr, s);
}

// ---------------------------------------------------------------- thumbnails of a mixed-size batch
// The staging workspace of llfe_thumbnail_pil_images is bounded: the staged host sources and
// the pre-pass results go through it in chunks of images on the one stream (a chunk's resample
// is ordered before the next chunk's copies).  256 MiB is seven 12 MP sources.
constexpr int64_t kThumbStageBudget = (int64_t)256 << 20;

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

bool valid_image_desc(const llfe_image_desc &d) {
    return d.data && valid_dims(1, d.height, d.width) && (d.row_stride == 0 || d.row_stride >= 3 * (int64_t)d.width);
}

// the plan of one distinct (h, w) of a call, with what the kernels need on top of it
struct ThumbPlan {
    int h = 0, w = 0;
    ThumbGeom g;
    LanczosPlan lz;
    int mode = kThumbCopy, tile_h = kThumbTileH;
    int64_t tab = 0;  // offset of [bh | kh | bv | kv] in the call's int32 table
    const char *err = nullptr;
    int64_t tab_size() const { return (int64_t)(lz.bh.size() + lz.kh.size() + lz.bv.size() + lz.kv.size()); }
};

// rows of the horizontal pass the tiles of `th` output rows need at most; -1 when a row of a
// tile reaches outside what the tile's first and last row span
int thumb_tile_rows(const LanczosPlan &p, int th) {
    int most = 0;
    for (int y0 = 0; y0 < p.oh; y0 += th) {
        const int y1 = std::min(p.oh, y0 + th) - 1;
        const int r0 = p.bv[2 * y0], r1 = p.bv[2 * y1] + p.bv[2 * y1 + 1];
        for (int y = y0; y <= y1; y++)
            if (p.bv[2 * y] < r0 || p.bv[2 * y] + p.bv[2 * y + 1] > r1) return -1;
        most = std::max(most, r1 - r0);
    }
    return most;
}

// Builds the plan and checks everything the kernels index with against the sizes and the
// kernels' compile-time bounds: nothing is launched on a plan that has not passed here.
void thumb_plan_build(ThumbPlan &P, int32_t max_w, int32_t max_h) {
    if (thumb_geometry(P.h, P.w, max_w, max_h, P.g) < 0) {
        P.err = "invalid thumbnail geometry";
        return;
    }
    if (!P.g.resized) return;
    const ThumbGeom &g = P.g;
    LanczosPlan &p = P.lz;
    lanczos_plan(g.rh, g.rw, g.oh, g.ow, g.reduced() ? g.box : nullptr, p);
    P.mode = (p.need_h ? kThumbH : 0) | (p.need_v ? kThumbV : 0);
    if (P.mode == kThumbCopy) return;
    if (!p.need_h) p.yfirst = 0;  // (bv is absolute then)
    // after the pre-pass the residual scale is below 4 (s / floor(s / 2) < 4), so ksize <= 25;
    // checked, not assumed
    if ((p.need_h && p.ksh > kThumbMaxK) || (p.need_v && p.ksv > kThumbMaxK)) {
        P.err = "filter wider than the kernel's bound";
        return;
    }
    for (int x = 0; x < g.ow; x++) {
        const int a = p.bh[2 * x], c = p.bh[2 * x + 1];
        if (a < 0 || c < 0 || c > p.ksh || (int64_t)a + c > g.rw) P.err = "horizontal bounds outside the source";
    }
    for (int y = 0; y < g.oh; y++) {
        const int64_t a = (int64_t)p.bv[2 * y] + p.yfirst;
        const int c = p.bv[2 * y + 1];
        if (a < 0 || c < 0 || c > p.ksv || a + c > g.rh) P.err = "vertical bounds outside the source";
    }
    if (p.need_h && !p.need_v && (p.yfirst < 0 || (int64_t)p.yfirst + g.oh > g.rh))
        P.err = "horizontal pass outside the source";
    if (P.err || P.mode != kThumbBoth) return;
    // the tallest tile whose rows fit the LDS budget
    for (int th = kThumbTileH; th >= 1; th /= 2) {
        const int rows = thumb_tile_rows(p, th);
        if (rows >= 0 && rows <= kThumbLdsRows) {
            P.tile_h = th;
            return;
        }
    }
    P.err = "no tile height fits the LDS budget";
}

int thumb_layout(const llfe_image_desc *images, int32_t n, int32_t max_w, int32_t max_h, llfe_thumb_out *outs,
                 int64_t *dst_bytes) {
    if (n < 0 || max_w <= 0 || max_h <= 0 || !dst_bytes || (n > 0 && (!images || !outs))) return LLFE_ERR_INVALID;
    for (int i = 0; i < n; i++)
        if (!valid_image_desc(images[i])) return LLFE_ERR_INVALID;
    int64_t end = 0;
    for (int i = 0; i < n; i++) {
        int32_t ow, oh;
        const int rc = llfe_thumbnail_size(images[i].width, images[i].height, max_w, max_h, &ow, &oh);
        if (rc < 0) return LLFE_ERR_INVALID;
        outs[i].offset = align16(end);
        outs[i].height = oh, outs[i].width = ow, outs[i].resized = rc, outs[i].pad_ = 0;
        end = outs[i].offset + (int64_t)oh * ow * 3;
    }
    *dst_bytes = end;
    return LLFE_OK;
}

int thumbnail_images(llfe_ctx *ctx, const llfe_image_desc *images, int n, int32_t max_w, int32_t max_h, uint8_t *dst,
                     const llfe_thumb_out *outs, hipStream_t s) {
    const auto t_plan = std::chrono::steady_clock::now();
    // one plan per distinct (h, w), built on the pool
    std::vector<ThumbPlan> plans;
    std::vector<int> plan_of((size_t)n);
    {
        std::map<std::pair<int, int>, int> seen;
        for (int i = 0; i < n; i++) {
            const auto key = std::make_pair(images[i].height, images[i].width);
            auto f = seen.find(key);
            if (f == seen.end()) {
                f = seen.emplace(key, (int)plans.size()).first;
                plans.emplace_back();
                plans.back().h = key.first, plans.back().w = key.second;
            }
            plan_of[i] = f->second;
        }
    }
    auto build = [&](int p, int) { thumb_plan_build(plans[p], max_w, max_h); };
    if (ctx->pool)
        ctx->pool->parallel_for((int)plans.size(), build);
    else
        for (size_t p = 0; p < plans.size(); p++) build((int)p, 0);
    int64_t tab_n = 0;
    for (ThumbPlan &P : plans) {
        if (P.err)
            return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_thumbnail_pil_images: %d x %d: %s", P.h, P.w, P.err);
        P.tab = tab_n;
        if (P.mode != kThumbCopy) tab_n += P.tab_size();
    }
    // per image: workspace bytes (a staged host source, the pre-pass result), work entries
    struct Item {
        int64_t stage = 0, red = 0, ws = 0;  // bytes; ws: offset in the chunk's workspace
        int64_t n_red = 0, n_lz = 0;
        bool direct = false;  // a host image that fits: one 2-D copy into dst
    };
    std::vector<Item> it((size_t)n);
    int64_t red_total = 0, lz_total = 0;
    for (int i = 0; i < n; i++) {
        const ThumbPlan &P = plans[plan_of[i]];
        const llfe_image_desc &d = images[i];
        Item &q = it[i];
        if (P.mode == kThumbCopy && !d.on_device) {
            q.direct = true;
            continue;
        }
        if (!d.on_device) q.stage = align16((int64_t)d.height * d.width * 3);
        if (P.g.reduced()) {
            q.red = align16((int64_t)P.g.rh * P.g.rw * 3);
            const int64_t rtx = ((int64_t)P.g.rw * 3 + kThumbReduceBytes - 1) / kThumbReduceBytes;
            q.n_red = rtx * ((P.g.rh + kThumbReduceRows - 1) / kThumbReduceRows);
        }
        q.n_lz = (int64_t)((P.g.ow + kThumbTileW - 1) / kThumbTileW) * ((P.g.oh + P.tile_h - 1) / P.tile_h);
        red_total += q.n_red, lz_total += q.n_lz;
    }
    if (red_total >= (1LL << 31) || lz_total >= (1LL << 31) || tab_n >= (1LL << 31))
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_thumbnail_pil_images: the batch needs too many tiles for one call");
    // chunks of consecutive images whose workspace fits the budget (one image always fits)
    int64_t budget = kThumbStageBudget;
    if (const char *e = getenv("LLFE_THUMB_STAGE_BYTES"); e && atoll(e) > 0) budget = atoll(e);  // (tests: many chunks)
    struct Chunk {
        int i0, i1;
        int64_t red0, red1, lz0, lz1;  // its entries of the two work tables
    };
    std::vector<Chunk> chunks;
    int64_t ws_bytes = 0;
    {
        int64_t used = 0, red_at = 0, lz_at = 0;
        Chunk c{0, 0, 0, 0, 0, 0};
        for (int i = 0; i < n; i++) {
            const int64_t need = it[i].stage + it[i].red;
            if (i > c.i0 && need > 0 && used + need > budget) {
                c.i1 = i, c.red1 = red_at, c.lz1 = lz_at;
                chunks.push_back(c);
                c = Chunk{i, i, red_at, red_at, lz_at, lz_at};
                used = 0;
            }
            it[i].ws = used;
            used += need;
            ws_bytes = std::max(ws_bytes, used);
            red_at += it[i].n_red, lz_at += it[i].n_lz;
        }
        c.i1 = n, c.red1 = red_at, c.lz1 = lz_at;
        chunks.push_back(c);
    }
    HIPCHK(ctx, ctx->d_thumb_ws.ensure((size_t)std::max<int64_t>(ws_bytes, 16)));
    // one pinned block: [int32 table | records | reduce work | resample work], one upload
    const int64_t o_rec = align16(tab_n * 4), o_red = o_rec + align16((int64_t)n * sizeof(ThumbRec)),
                  o_lz = o_red + align16(red_total * sizeof(ThumbWork)),
                  blk = o_lz + align16(lz_total * sizeof(ThumbWork));
    HIPCHK(ctx, ctx->h_thumb_tab.ensure((size_t)blk));
    HIPCHK(ctx, ctx->d_thumb_tab.ensure((size_t)blk));
    uint8_t *hb = ctx->h_thumb_tab.p, *db = ctx->d_thumb_tab.p;
    int32_t *tab = (int32_t *)hb;
    for (const ThumbPlan &P : plans) {
        if (P.mode == kThumbCopy) continue;
        int32_t *o = tab + P.tab;
        for (const std::vector<int32_t> *v : {&P.lz.bh, &P.lz.kh, &P.lz.bv, &P.lz.kv}) {
            std::memcpy(o, v->data(), v->size() * sizeof(int32_t));
            o += v->size();
        }
    }
    ThumbRec *recs = (ThumbRec *)(hb + o_rec);
    ThumbWork *w_red = (ThumbWork *)(hb + o_red), *w_lz = (ThumbWork *)(hb + o_lz);
    double bytes_red = 0, bytes_lz = 0;
    for (int i = 0; i < n; i++) {
        const ThumbPlan &P = plans[plan_of[i]];
        const llfe_image_desc &d = images[i];
        const Item &q = it[i];
        ThumbRec &r = recs[i];
        std::memset(&r, 0, sizeof r);
        if (q.direct) continue;
        const int64_t pitch = d.row_stride ? d.row_stride : (int64_t)d.width * 3;
        uint8_t *ws = ctx->d_thumb_ws.p + q.ws;
        r.rsrc = d.on_device ? d.data : ws;
        r.rsrc_stride = d.on_device ? pitch : (int64_t)d.width * 3;
        r.red = P.g.reduced() ? ws + q.stage : nullptr;
        r.src = P.g.reduced() ? r.red : r.rsrc;
        r.src_stride = P.g.reduced() ? (int64_t)P.g.rw * 3 : r.rsrc_stride;
        r.dst = dst + outs[i].offset;
        r.h = d.height, r.w = d.width, r.rh = P.g.rh, r.rw = P.g.rw, r.oh = P.g.oh, r.ow = P.g.ow;
        r.fx = P.g.fx, r.fy = P.g.fy;
        r.mode = P.mode, r.ksh = P.lz.ksh, r.ksv = P.lz.ksv, r.yfirst = P.lz.yfirst;
        r.bh = (int32_t)P.tab, r.kh = r.bh + (int32_t)P.lz.bh.size(), r.bv = r.kh + (int32_t)P.lz.kh.size();
        r.kv = r.bv + (int32_t)P.lz.bv.size();
        r.tile_h = P.tile_h, r.tiles_x = (P.g.ow + kThumbTileW - 1) / kThumbTileW;
        r.rtiles_x = (int32_t)(((int64_t)P.g.rw * 3 + kThumbReduceBytes - 1) / kThumbReduceBytes);
        for (int64_t t = 0; t < q.n_red; t++) *w_red++ = ThumbWork{i, (int32_t)t};
        for (int64_t t = 0; t < q.n_lz; t++) *w_lz++ = ThumbWork{i, (int32_t)t};
        if (q.n_red) bytes_red += (double)d.height * d.width * 3 + (double)P.g.rh * P.g.rw * 3;
        bytes_lz += (double)P.g.rh * P.g.rw * 3 + (double)P.g.oh * P.g.ow * 3;
    }
    if (ctx->prof.on) {  // the host plan beside the kernels in llfe_kernel_stats
        Profiler::Stat &st = ctx->prof.stats[ctx->prof.kid("thumb_plan_host")];
        st.launches++;
        st.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_plan).count();
    }
    HIPCHK(ctx, hipMemcpyAsync(db, hb, (size_t)blk, hipMemcpyHostToDevice, s));
    const ThumbRec *d_recs = (const ThumbRec *)(db + o_rec);
    const ThumbWork *d_red = (const ThumbWork *)(db + o_red), *d_lz = (const ThumbWork *)(db + o_lz);
    const double share_red = red_total ? bytes_red / (double)red_total : 0, share_lz = lz_total ? bytes_lz / (double)lz_total : 0;
    for (const Chunk &c : chunks) {
        StageSlotScope tag(ctx->prof);
        for (int i = c.i0; i < c.i1; i++) {
            const llfe_image_desc &d = images[i];
            if (d.on_device) continue;
            const size_t pitch = d.row_stride ? (size_t)d.row_stride : (size_t)d.width * 3, row = (size_t)d.width * 3;
            uint8_t *to = it[i].direct ? dst + outs[i].offset : ctx->d_thumb_ws.p + it[i].ws;
            HIPCHK(ctx, hipMemcpy2DAsync(to, row, d.data, pitch, row, d.height, hipMemcpyHostToDevice, s));
        }
        if (c.red1 > c.red0)
            TIMED(ctx, s, "k_thumb_reduce", share_red * (double)(c.red1 - c.red0),
                  launch_thumb_reduce(d_recs, d_red + c.red0, (int)(c.red1 - c.red0), s));
        if (c.lz1 > c.lz0)
            TIMED(ctx, s, "k_thumb_lanczos", share_lz * (double)(c.lz1 - c.lz0),
                  launch_thumb_lanczos(d_recs, d_lz + c.lz0, (int)(c.lz1 - c.lz0), (const int32_t *)db, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));  // the pinned block and the workspace are free again
    ctx->prof.collect(Profiler::kStageSlot);
    return LLFE_OK;
}

}  // namespace

extern "C" {

int llfe_resize_lanczos_pil(llfe_ctx *ctx, const uint8_t *src, int32_t h, int32_t w, int32_t ch, uint8_t *dst,
                            int32_t out_h, int32_t out_w, const double *box, llfe_stream stream) {
    if (!ctx || !src || !dst || h <= 0 || w <= 0 || ch <= 0 || out_h <= 0 || out_w <= 0) return LLFE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return resize_lanczos_n(ctx, src, 1, h, w, ch, dst, out_h, out_w, box, (hipStream_t)stream);
}

// PIL Image.thumbnail's preserve_aspect_ratio (Python float semantics).  Returns 1
// and the new size when a resize happens, 0 when the image already fits.
int llfe_thumbnail_size(int32_t w, int32_t h, int32_t max_w, int32_t max_h, int32_t *out_w, int32_t *out_h) {
    if (w <= 0 || h <= 0 || max_w <= 0 || max_h <= 0 || !out_w || !out_h) return LLFE_ERR_INVALID;
    *out_w = w;
    *out_h = h;
    int64_t x = max_w, y = max_h;
    if (x >= w && y >= h) return 0;
    const double aspect = (double)w / (double)h;
    if ((double)x / (double)y >= aspect) {
        double num = (double)y * aspect;
        int64_t f = (int64_t)std::floor(num), c = (int64_t)std::ceil(num);
        double kf = std::fabs(aspect - (double)f / (double)y), kc = std::fabs(aspect - (double)c / (double)y);
        x = std::max<int64_t>(kc < kf ? c : f, 1);  // min(floor, ceil, key=...) keeps floor on ties
    } else {
        double num = (double)x / aspect;
        int64_t f = (int64_t)std::floor(num), c = (int64_t)std::ceil(num);
        auto key = [&](int64_t n) { return n == 0 ? 0.0 : std::fabs(aspect - (double)x / (double)n); };
        y = std::max<int64_t>(key(c) < key(f) ? c : f, 1);
    }
    *out_w = (int32_t)x;
    *out_h = (int32_t)y;
    return (x != w || y != h) ? 1 : 0;
}

// ImageProcessor.auto_process_image's resize: PIL thumbnail((max_w, max_h), LANCZOS,
// reducing_gap=2.0) on a device u8 HWC image (image_processor.py:221-224).  dst must hold
// out_h * out_w * ch bytes (at most h * w * ch).
int llfe_thumbnail_pil(llfe_ctx *ctx, const uint8_t *src, int32_t h, int32_t w, int32_t ch, int32_t max_w,
                       int32_t max_h, uint8_t *dst, int64_t dst_capacity, int32_t *out_h, int32_t *out_w,
                       llfe_stream stream) {
    if (!ctx || !src || !dst || !out_h || !out_w || ch <= 0) return LLFE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return thumbnail_n(ctx, src, 1, h, w, ch, max_w, max_h, dst, dst_capacity, out_h, out_w, (hipStream_t)stream);
}

int llfe_thumbnail_pil_batch(llfe_ctx *ctx, const uint8_t *src, int32_t n, int32_t h, int32_t w, int32_t ch,
                             int32_t max_w, int32_t max_h, uint8_t *dst, int64_t dst_capacity, int32_t *out_h,
                             int32_t *out_w, llfe_stream stream) {
    if (!ctx || n < 0 || (n > 0 && (!src || !dst)) || !out_h || !out_w || ch <= 0 || n > 65535)
        return LLFE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n == 0) return llfe_thumbnail_size(w, h, max_w, max_h, out_w, out_h) < 0 ? LLFE_ERR_INVALID : LLFE_OK;
    return thumbnail_n(ctx, src, n, h, w, ch, max_w, max_h, dst, dst_capacity, out_h, out_w, (hipStream_t)stream);
}

int llfe_thumbnail_images_layout(const llfe_image_desc *images, int32_t n, int32_t max_w, int32_t max_h,
                                 llfe_thumb_out *outs, int64_t *dst_bytes) {
    return thumb_layout(images, n, max_w, max_h, outs, dst_bytes);
}

// Image.thumbnail of n images of any sizes in one device pass: one plan per distinct size, one
// upload of every table, one reduce and one resample launch per staging chunk
// (thumb_images.hip), one synchronisation at the end
int llfe_thumbnail_pil_images(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, int32_t max_w,
                              int32_t max_h, uint8_t *dst, int64_t dst_capacity, llfe_thumb_out *outs,
                              llfe_stream stream) {
    if (!ctx) return LLFE_ERR_INVALID;
    int64_t total = 0;
    if (thumb_layout(images, n, max_w, max_h, outs, &total) != LLFE_OK || (n > 0 && !dst) || dst_capacity < 0)
        return ctx->fail(LLFE_ERR_INVALID, "llfe_thumbnail_pil_images: bad arguments or an invalid image descriptor");
    if (n == 0) return LLFE_OK;
    if (total > dst_capacity)
        return ctx->fail(LLFE_ERR_CAPACITY, "llfe_thumbnail_pil_images: dst holds %lld bytes, the layout needs %lld",
                         (long long)dst_capacity, (long long)total);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return thumbnail_images(ctx, images, n, max_w, max_h, dst, outs, (hipStream_t)stream);
}

int llfe_thumbnail_images_tiling(int32_t *tile_w, int32_t *tile_h, int32_t *lds_rows, int32_t *max_ksize) {
    if (!tile_w || !tile_h || !lds_rows || !max_ksize) return LLFE_ERR_INVALID;
    *tile_w = kThumbTileW, *tile_h = kThumbTileH, *lds_rows = kThumbLdsRows, *max_ksize = kThumbMaxK;
    return LLFE_OK;
}

// cv2.resize (validate_and_preprocess_image, utils.py:118-143); tables built on the host
// exactly as OpenCV builds them, one kernel evaluates the output (cvresize.hip)
int llfe_resize_cv(llfe_ctx *ctx, const uint8_t *src, int32_t h, int32_t w, int32_t ch, uint8_t *dst, int32_t out_h,
                   int32_t out_w, int32_t interpolation, llfe_stream stream) {
    if (!ctx || !src || !dst || h <= 0 || w <= 0 || ch <= 0 || out_h <= 0 || out_w <= 0) return LLFE_ERR_INVALID;
    if (ch > 4) return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_resize_cv: ch > 4");
    CvResizePlan plan;
    if (cv_resize_plan(h, w, ch, out_h, out_w, interpolation, plan) != 0)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_resize_cv: interpolation %d not supported", interpolation);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int32_t *dtab = nullptr;
    if (!plan.tab.empty()) {
        HIPCHK(ctx, ctx->d_coef.ensure(plan.tab.size()));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef.p, plan.tab.data(), plan.tab.size() * sizeof(int32_t),
                                   hipMemcpyHostToDevice, s));
        dtab = ctx->d_coef.p;
    }
    HIPCHK(ctx, launch_cv_resize(plan, src, dst, dtab, s));
    HIPCHK(ctx, hipStreamSynchronize(s));  // the host table dies here
    return LLFE_OK;
}

int llfe_preprocess_size(int32_t w, int32_t h, int32_t mode, int32_t *out_w, int32_t *out_h, int32_t *interpolation) {
    if (w <= 0 || h <= 0 || !out_w || !out_h || !interpolation) return LLFE_ERR_INVALID;
    int max_dim, interp;
    switch (mode) {
    case LLFE_PRE_AUTO: max_dim = 2000, interp = LLFE_CV_INTER_AREA; break;
    case LLFE_PRE_HIGH_QUALITY: max_dim = 4000, interp = LLFE_CV_INTER_LANCZOS4; break;
    case LLFE_PRE_PERFORMANCE: max_dim = 1000, interp = LLFE_CV_INTER_LINEAR; break;
    case LLFE_PRE_NONE: return 0;
    default: return LLFE_ERR_INVALID;
    }
    const int m = std::max(w, h);
    if (m <= max_dim) return 0;
    const double scale = (double)max_dim / m;  // Python: max_dim / max(h, w)
    *out_w = (int32_t)(w * scale);             // int(w * scale): truncation toward 0
    *out_h = (int32_t)(h * scale);
    *interpolation = interp;
    return 1;
}

int llfe_reduce_pil(llfe_ctx *ctx, const uint8_t *src, int32_t h, int32_t w, int32_t ch, int32_t fx, int32_t fy,
                    uint8_t *dst, llfe_stream stream) {
    if (!ctx || !src || !dst || h <= 0 || w <= 0 || ch <= 0 || fx <= 0 || fy <= 0) return LLFE_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int rw = (w + fx - 1) / fx, rh = (h + fy - 1) / fy;
    HIPCHK(ctx, launch_reduce(src, w, ch, 0, 0, w, h, fx, fy, dst, rw, rh, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return LLFE_OK;
}

int llfe_text_size(int32_t h, int32_t w, int32_t *out_h, int32_t *out_w) {
    if (h <= 0 || w <= 0 || !out_h || !out_w) return LLFE_ERR_INVALID;
    if (h < 30 || w < 100) {  // scale = max(2, 300 / width, 100 / height) (Python floats)
        const double sc = std::max(std::max(2.0, 300.0 / w), 100.0 / h);
        if (w * sc >= 2147483647.0 || h * sc >= 2147483647.0) return LLFE_ERR_UNSUPPORTED;
        *out_w = (int32_t)std::lrint(w * sc);  // saturate_cast<int>(double): round half even
        *out_h = (int32_t)std::lrint(h * sc);
        return 1;
    }
    *out_h = h;
    *out_w = w;
    return 0;
}

// TextExtractor.preprocess_image (text_extractor.py:15-46): gray, INTER_CUBIC upscale
// of small images (cvresize.hip), Otsu binary and the mean > 127 inversion (text.hip)
int llfe_text_binary(llfe_ctx *ctx, const uint8_t *img, int32_t h, int32_t w, int32_t channels, uint8_t *out,
                     int32_t *threshold, llfe_stream stream) {
    if (!ctx || !img || !out || h <= 0 || w <= 0) return LLFE_ERR_INVALID;
    if (channels != 1 && channels != 3 && channels != 4)
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_text_binary: %d channels (1, 3 or 4)", channels);
    int32_t oh, ow;
    const int up = llfe_text_size(h, w, &oh, &ow);
    if (up < 0 || !valid_dims(1, h, w) || !valid_dims(1, oh, ow))
        return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_text_binary: %d x %d (-> %d x %d) pixels", h, w, oh, ow);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)h * w, n2 = (long long)oh * ow;
    HIPCHK(ctx, ctx->d_text.ensure((size_t)(n + (up ? n2 : 0))));
    HIPCHK(ctx, ctx->d_text_hist.ensure(258));
    uint8_t *gray = ctx->d_text.p, *g = gray;
    HIPCHK(ctx, launch_text_gray(img, n, channels, gray, s));
    if (up) {
        const double sc = std::max(std::max(2.0, 300.0 / w), 100.0 / h);
        CvResizePlan plan;
        if (cv_resize_plan_scaled(h, w, 1, oh, ow, sc, sc, kCvInterCubic, plan) != 0)
            return ctx->fail(LLFE_ERR_UNSUPPORTED, "llfe_text_binary: resize plan");
        HIPCHK(ctx, ctx->d_coef.ensure(plan.tab.size()));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef.p, plan.tab.data(), plan.tab.size() * sizeof(int32_t),
                                   hipMemcpyHostToDevice, s));
        g = gray + n;
        HIPCHK(ctx, launch_cv_resize(plan, gray, g, ctx->d_coef.p, s));
        HIPCHK(ctx, hipStreamSynchronize(s));  // the host table dies with `plan`
    }
    HIPCHK(ctx, launch_text_otsu_binary(g, n2, ctx->d_text_hist.p, out, s));
    if (threshold) {
        unsigned long long t = 0;
        HIPCHK(ctx, hipMemcpyAsync(&t, ctx->d_text_hist.p + 256, sizeof t, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        *threshold = (int32_t)t;
    } else {
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return LLFE_OK;
}

}  // extern "C"
