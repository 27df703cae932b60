// C ABI of libllfe.so (include/llfe.h): Pillow LANCZOS resize / thumbnail / reduce, cv2.resize
// and the text binary.
#include <cmath>

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

// Image.resize(size, LANCZOS, box) of n same-size packed device images
int resize_lanczos_n(llfe_ctx *ctx, const uint8_t *src, int n, int32_t h, int32_t w, int32_t ch, uint8_t *dst,
                     int32_t out_h, int32_t out_w, const double *box, hipStream_t s) {
    // Pillow hands the box of Image.resize to its C code as four 32-bit floats: w / 3 arrives there
    // rounded to float32, and the coefficients follow from that value
    auto f32 = [](double v) { return (double)(float)v; };
    double bx0 = box ? f32(box[0]) : 0, by0 = box ? f32(box[1]) : 0, bx1 = box ? f32(box[2]) : w,
           by1 = box ? f32(box[3]) : h;
    bool need_h = out_w != w || bx0 != 0 || bx1 != out_w;
    bool need_v = out_h != h || by0 != 0 || by1 != out_h;
    std::vector<int32_t> bh, kh, bv, kv;
    int ksh = pil_coeffs(w, bx0, bx1, out_w, bh, kh);
    int ksv = pil_coeffs(h, by0, by1, out_h, bv, kv);
    int yfirst = bv[0], ylast = bv[2 * out_h - 2] + bv[2 * out_h - 1];
    // coefficient block: [bh | kh | bv | kv]
    size_t nb = bh.size() + kh.size() + bv.size() + kv.size();
    HIPCHK(ctx, ctx->d_coef.ensure(nb));
    std::vector<int32_t> all;
    all.reserve(nb);
    if (need_h)
        for (int i = 0; i < out_h; i++) bv[2 * i] -= yfirst;
    all.insert(all.end(), bh.begin(), bh.end());
    all.insert(all.end(), kh.begin(), kh.end());
    all.insert(all.end(), bv.begin(), bv.end());
    all.insert(all.end(), kv.begin(), kv.end());
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_coef.p, all.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int32_t *dbh = ctx->d_coef.p, *dkh = dbh + bh.size(), *dbv = dkh + kh.size(), *dkv = dbv + bv.size();
    const long long in_img = (long long)h * w * ch, out_img = (long long)out_h * out_w * ch;
    if (!need_h && !need_v) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)n * in_img, hipMemcpyDeviceToDevice, s));
    } else if (need_h && !need_v) {
        HIPCHK(ctx, launch_resize_h(src, h, w, ch, yfirst, ylast - yfirst, dst, out_w, dbh, dkh, ksh, s, n, in_img,
                                    out_img));
    } else if (!need_h) {
        HIPCHK(ctx, launch_resize_v(src, w, ch, dst, out_h, dbv, dkv, ksv, s, n, in_img, out_img));
    } else {
        const int rows = ylast - yfirst;
        const long long tmp_img = (long long)rows * out_w * ch;
        HIPCHK(ctx, ctx->d_rsz_tmp.ensure((size_t)n * tmp_img));
        HIPCHK(ctx, launch_resize_h(src, h, w, ch, yfirst, rows, ctx->d_rsz_tmp.p, out_w, dbh, dkh, ksh, s, n, in_img,
                                    tmp_img));
        HIPCHK(ctx, launch_resize_v(ctx->d_rsz_tmp.p, out_w, ch, dst, out_h, dbv, dkv, ksv, s, n, tmp_img, out_img));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));  // host coefficient vectors die here
    return LLFE_OK;
}

// thumbnail((max_w, max_h), LANCZOS) incl. the reducing_gap=2.0 reduce() pre-pass, n images
int thumbnail_n(llfe_ctx *ctx, const uint8_t *src, int n, int32_t h, int32_t w, int32_t ch, int32_t max_w,
                int32_t max_h, uint8_t *dst, int64_t dst_capacity, int32_t *out_h, int32_t *out_w, hipStream_t s) {
    int32_t ow, oh;
    int rc = llfe_thumbnail_size(w, h, max_w, max_h, &ow, &oh);
    if (rc < 0) return ctx->fail(rc, "invalid thumbnail geometry");
    if ((int64_t)n * ow * oh * ch > dst_capacity) return ctx->fail(LLFE_ERR_CAPACITY, "thumbnail dst too small");
    *out_w = ow;
    *out_h = oh;
    if (rc == 0) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)n * h * w * ch, hipMemcpyDeviceToDevice, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return LLFE_OK;
    }
    // Image.resize(size, LANCZOS, box=None, reducing_gap=2.0)
    const double gap = 2.0;
    int fx = (int)((double)w / ow / gap), fy = (int)((double)h / oh / gap);
    if (fx < 1) fx = 1;
    if (fy < 1) fy = 1;
    if (fx > 1 || fy > 1) {
        // _get_safe_box of the full image is the full image itself
        const int rw = (w + fx - 1) / fx, rh = (h + fy - 1) / fy;
        const long long red_img = (long long)rw * rh * ch;
        HIPCHK(ctx, ctx->d_rsz_src.ensure((size_t)n * red_img));
        HIPCHK(ctx, launch_reduce(src, w, ch, 0, 0, w, h, fx, fy, ctx->d_rsz_src.p, rw, rh, s, n,
                                  (long long)h * w * ch, red_img));
        const double box[4] = {0.0, 0.0, (double)w / fx, (double)h / fy};
        return resize_lanczos_n(ctx, ctx->d_rsz_src.p, n, rh, rw, ch, dst, oh, ow, box, s);
    }
    return resize_lanczos_n(ctx, src, n, h, w, ch, dst, oh, ow, nullptr, s);
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
