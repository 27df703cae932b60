// cv2.resize of a batch of BGR images of any sizes (llfe_preprocess_images,
// llfe_resize_cv_images): cvresize.hip's arithmetic, ragged.
//
// The host builds one record per image (CvImgRec: pointers, row stride, sizes, the plan kind,
// the offsets of its plan's tables in one int32 table) and one work table of (image, tile)
// entries per plan kind; a workgroup takes one entry.  Nothing is shared between workgroups and
// nothing is accumulated across them: no atomics.  Every index below derives from a record whose
// tables, tile height and arm the host checked against the image sizes and the LDS budgets
// before the launch (cv_images_plan_check, llfe_preprocess_images.cpp).
//
//   k_cv_images_area       resizeArea_ on an output tile of kCvTileW pixels x tile_h rows.  The
//                          tile's slice of the x table and of the y table sit in LDS; the source
//                          rows the tile needs come to LDS in chunks, a dword per lane along the
//                          row; the horizontal pass runs once per (source row, output pixel) into
//                          an LDS float32 row buffer (OpenCV's own), in table order with a separate
//                          multiply and add; the vertical pass runs from there, a lane per output
//                          byte.  Two output rows that share a source row read the one buffer row.
//   k_cv_images_area_fast  resizeAreaFast_: the tile's fy * tile_h source rows in LDS, a lane per
//                          output pixel.
//   k_cv_images_generic    resizeGeneric_ for 2 (LINEAR, AREA upscale) and 8 (LANCZOS4) taps, a
//                          lane per output pixel, from global memory.
//   k_cv_images_copy       an image the rule leaves, copied to its place.
// An image whose tile does not fit the budgets at any tile height (a scale above about 14 in x)
// takes the arm of the same kernel that reads its taps from global memory (arm == kCvArmGlobal).
#include "llfe_internal.h"

namespace llfe {
namespace {

constexpr int CT = 256;
constexpr int ROWB = kCvTileW * 3;  // bytes (and row-buffer floats) of a tile row

__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int rint_sat8(float v) { return sat8((int)__builtin_rintf(v)); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// nrows rows of `span` bytes, the first at g0, `stride` bytes apart, into LDS rows of `pitch`
// bytes (a multiple of 4, at least span + 3): a row keeps its address modulo 4, so that the
// dwords inside it are loaded as dwords; the bytes of a row's first and last dword that lie
// outside the row are not read
__device__ __forceinline__ void stage_rows(const uint8_t *__restrict__ g0, size_t stride, int nrows, int span,
                                           int pitch, uint32_t *__restrict__ lds, int tid) {
    const int nw = pitch >> 2;
    for (int e = tid; e < nrows * nw; e += CT) {
        const int rr = e / nw, wi = e - rr * nw;
        const uint8_t *g = g0 + (size_t)rr * stride;
        const int lead = (int)((uintptr_t)g & 3);
        const int b0 = wi * 4 - lead;  // the dword's first byte, relative to the row
        if (b0 >= span) continue;
        uint32_t v;
        if (b0 >= 0 && b0 + 4 <= span) {
            v = *(const uint32_t *)(g + b0);
        } else {
            v = 0;
            for (int k = 0; k < 4; k++)
                if (b0 + k >= 0 && b0 + k < span) v |= (uint32_t)g[b0 + k] << (8 * k);
        }
        lds[e] = v;
    }
}

// ---------------------------------------------------------------------------- AREA
__global__ __launch_bounds__(CT) void k_cv_images_area(const CvImgRec *__restrict__ recs,
                                                       const CvImgWork *__restrict__ work,
                                                       const int32_t *__restrict__ tab) {
    __shared__ float s_buf[kCvLdsRows * ROWB];
    __shared__ __attribute__((aligned(16))) uint32_t s_src[kCvStageBytes / 4];
    __shared__ int32_t s_xp[kCvMaxPairs * 2];
    __shared__ int32_t s_xs[kCvTileW + 1];
    __shared__ int32_t s_yp[kCvMaxYPairs * 2];
    __shared__ int32_t s_ys[kCvTileH + 1];
    const CvImgWork wk = work[blockIdx.x];
    const CvImgRec &r = recs[wk.image];
    const int tid = threadIdx.x;
    const int tx = wk.tile % r.tiles_x, ty = wk.tile / r.tiles_x;
    const int x0 = tx * kCvTileW, nx = min(kCvTileW, r.ow - x0);
    const int y0 = ty * r.tile_h, ny = min(r.tile_h, r.oh - y0);
    const size_t dpitch = (size_t)r.ow * 3;
    uint8_t *__restrict__ dst = r.dst + (size_t)y0 * dpitch + (size_t)x0 * 3;
    const uint8_t *__restrict__ src = r.src;
    const size_t stride = (size_t)r.src_stride;
    const int32_t *__restrict__ xt = tab + r.xt;  // [ow + 1] starts, then (si, alpha) pairs
    const int32_t *__restrict__ yt = tab + r.yt;  // [oh + 1] starts, then (row, beta) pairs
    const int32_t *__restrict__ xp = xt + (r.ow + 1), *__restrict__ yp = yt + (r.oh + 1);

    if (r.arm == kCvArmGlobal) {  // k_cv_area, a lane per output pixel
        for (int e = tid; e < ny * kCvTileW; e += CT) {
            const int y = e / kCvTileW, xx = e - y * kCvTileW;
            if (xx >= nx) continue;
            const int dy = y0 + y, dx = x0 + xx;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            for (int j = yt[dy]; j < yt[dy + 1]; j++) {
                const uint8_t *S = src + (size_t)yp[2 * j] * stride;
                const float beta = __int_as_float(yp[2 * j + 1]);
                float b0 = 0.f, b1 = 0.f, b2 = 0.f;
                for (int k = xt[dx]; k < xt[dx + 1]; k++) {
                    const int si = xp[2 * k];
                    const float a = __int_as_float(xp[2 * k + 1]);
                    b0 = __fadd_rn(b0, __fmul_rn((float)S[si], a));
                    b1 = __fadd_rn(b1, __fmul_rn((float)S[si + 1], a));
                    b2 = __fadd_rn(b2, __fmul_rn((float)S[si + 2], a));
                }
                a0 = __fadd_rn(a0, __fmul_rn(beta, b0));
                a1 = __fadd_rn(a1, __fmul_rn(beta, b1));
                a2 = __fadd_rn(a2, __fmul_rn(beta, b2));
            }
            uint8_t *o = dst + (size_t)y * dpitch + xx * 3;
            o[0] = (uint8_t)rint_sat8(a0), o[1] = (uint8_t)rint_sat8(a1), o[2] = (uint8_t)rint_sat8(a2);
        }
        return;
    }

    // the tile's slices of the tables
    const int kx0 = xt[x0], nkx = xt[x0 + nx] - kx0;
    const int ky0 = yt[y0], nky = yt[y0 + ny] - ky0;
    for (int e = tid; e < nkx * 2; e += CT) s_xp[e] = xp[2 * (size_t)kx0 + e];
    for (int e = tid; e <= nx; e += CT) s_xs[e] = xt[x0 + e] - kx0;
    for (int e = tid; e < nky * 2; e += CT) s_yp[e] = yp[2 * (size_t)ky0 + e];
    for (int e = tid; e <= ny; e += CT) s_ys[e] = yt[y0 + e] - ky0;
    // the source rectangle: rows [r0, r1], bytes [c0, c1) of each (tables ascend)
    const int r0 = yp[2 * ky0], r1 = yp[2 * (ky0 + nky - 1)];
    const int c0 = xp[2 * kx0], c1 = xp[2 * (kx0 + nkx - 1)] + 3;
    const int nrows = r1 - r0 + 1, span = c1 - c0;
    const int pitch = (span + 6) & ~3;
    const int per = kCvStageBytes / pitch;  // rows of one chunk
    for (int ra = 0; ra < nrows; ra += per) {
        const int nr = min(per, nrows - ra);
        __syncthreads();  // the tables are in place; the chunk before is consumed
        stage_rows(src + (size_t)(r0 + ra) * stride + c0, stride, nr, span, pitch, s_src, tid);
        __syncthreads();
        const uint8_t *sb = (const uint8_t *)s_src;
        for (int e = tid; e < nr * kCvTileW; e += CT) {
            const int rr = e / kCvTileW, xx = e - rr * kCvTileW;
            if (xx >= nx) continue;
            const int lead = (int)((uintptr_t)(src + (size_t)(r0 + ra + rr) * stride + c0) & 3);
            const int off = rr * pitch + lead - c0;  // of source byte 0 of the row in the chunk
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;
            for (int k = s_xs[xx]; k < s_xs[xx + 1]; k++) {
                const uint8_t *S = sb + (off + s_xp[2 * k]);
                const float a = __int_as_float(s_xp[2 * k + 1]);
                b0 = __fadd_rn(b0, __fmul_rn((float)S[0], a));
                b1 = __fadd_rn(b1, __fmul_rn((float)S[1], a));
                b2 = __fadd_rn(b2, __fmul_rn((float)S[2], a));
            }
            float *o = s_buf + (ra + rr) * ROWB + xx * 3;
            o[0] = b0, o[1] = b1, o[2] = b2;
        }
    }
    __syncthreads();
    const int nb = nx * 3;
    for (int e = tid; e < ny * ROWB; e += CT) {
        const int y = e / ROWB, b = e - y * ROWB;
        if (b >= nb) continue;
        float acc = 0.f;
        for (int j = s_ys[y]; j < s_ys[y + 1]; j++)
            acc = __fadd_rn(acc, __fmul_rn(__int_as_float(s_yp[2 * j + 1]), s_buf[(s_yp[2 * j] - r0) * ROWB + b]));
        dst[(size_t)y * dpitch + b] = (uint8_t)rint_sat8(acc);
    }
}

// ---------------------------------------------------------------------------- AREA_FAST
// one output pixel of k_cv_area_fast from rows `pitch_of(row)` apart: S(yy) is row sy0 + yy
template <typename RowFn>
__device__ __forceinline__ void area_fast_pixel(RowFn row, int h, int w, int fx, int fy, int dy, int dx,
                                                uint8_t *__restrict__ o) {
    const int sy0 = dy * fy, sx0 = dx * fx;
    if (sy0 >= h) {
        o[0] = o[1] = o[2] = 0;
        return;
    }
    const bool full = sy0 + fy <= h && dx < w / fx;
    const bool fast2 = fx == 2 && fy == 2;
    const float scale = 1.f / (float)(fx * fy);
    int s0 = 0, s1 = 0, s2 = 0, count = 0;
    for (int yy = 0; yy < fy && sy0 + yy < h; yy++) {
        const uint8_t *R = row(yy);
        for (int xx = 0; xx < fx && sx0 + xx < w; xx++) {
            s0 += R[xx * 3], s1 += R[xx * 3 + 1], s2 += R[xx * 3 + 2];
            count++;
        }
    }
    if (full) {
        if (fast2) {
            o[0] = (uint8_t)((s0 + 2) >> 2), o[1] = (uint8_t)((s1 + 2) >> 2), o[2] = (uint8_t)((s2 + 2) >> 2);
        } else {
            o[0] = (uint8_t)rint_sat8((float)s0 * scale), o[1] = (uint8_t)rint_sat8((float)s1 * scale);
            o[2] = (uint8_t)rint_sat8((float)s2 * scale);
        }
    } else if (count) {
        o[0] = (uint8_t)rint_sat8((float)s0 / (float)count), o[1] = (uint8_t)rint_sat8((float)s1 / (float)count);
        o[2] = (uint8_t)rint_sat8((float)s2 / (float)count);
    } else {
        o[0] = o[1] = o[2] = 0;
    }
}

__global__ __launch_bounds__(CT) void k_cv_images_area_fast(const CvImgRec *__restrict__ recs,
                                                            const CvImgWork *__restrict__ work) {
    __shared__ __attribute__((aligned(16))) uint32_t s_src[kCvFastStageBytes / 4];
    const CvImgWork wk = work[blockIdx.x];
    const CvImgRec &r = recs[wk.image];
    const int tid = threadIdx.x;
    const int tx = wk.tile % r.tiles_x, ty = wk.tile / r.tiles_x;
    const int x0 = tx * kCvTileW, nx = min(kCvTileW, r.ow - x0);
    const int y0 = ty * r.tile_h, ny = min(r.tile_h, r.oh - y0);
    const size_t dpitch = (size_t)r.ow * 3;
    uint8_t *__restrict__ dst = r.dst + (size_t)y0 * dpitch + (size_t)x0 * 3;
    const uint8_t *__restrict__ src = r.src;
    const size_t stride = (size_t)r.src_stride;
    const int h = r.h, w = r.w, fx = r.fx, fy = r.fy;

    if (r.arm == kCvArmGlobal) {
        for (int e = tid; e < ny * kCvTileW; e += CT) {
            const int y = e / kCvTileW, xx = e - y * kCvTileW;
            if (xx >= nx) continue;
            const int dy = y0 + y, dx = x0 + xx;
            area_fast_pixel([&](int yy) { return src + (size_t)(dy * fy + yy) * stride + (size_t)dx * fx * 3; }, h, w,
                            fx, fy, dy, dx, dst + (size_t)y * dpitch + xx * 3);
        }
        return;
    }
    // source rows [ra, rb), pixels [ca, cb) of each, clipped to the image
    const int ra = min(y0 * fy, h), rb = min((y0 + ny) * fy, h);
    const int ca = min(x0 * fx, w), cb = min((x0 + nx) * fx, w);
    const int span = (cb - ca) * 3, pitch = (span + 6) & ~3;
    if (rb > ra && span > 0) stage_rows(src + (size_t)ra * stride + (size_t)ca * 3, stride, rb - ra, span, pitch, s_src, tid);
    __syncthreads();
    const uint8_t *sb = (const uint8_t *)s_src;
    for (int e = tid; e < ny * kCvTileW; e += CT) {
        const int y = e / kCvTileW, xx = e - y * kCvTileW;
        if (xx >= nx) continue;
        const int dy = y0 + y, dx = x0 + xx;
        area_fast_pixel(
            [&](int yy) {
                const int row = dy * fy + yy;
                const int lead = (int)((uintptr_t)(src + (size_t)row * stride + (size_t)ca * 3) & 3);
                return sb + (row - ra) * pitch + lead + (dx * fx - ca) * 3;
            },
            h, w, fx, fy, dy, dx, dst + (size_t)y * dpitch + xx * 3);
    }
}

// ---------------------------------------------------------------------------- GENERIC
// xs = [xofs px (ow)] [alpha (ow * KS)], ys = [yofs (oh)] [beta (oh * KS)]
template <int KS>
__device__ __forceinline__ void generic_pixel(const CvImgRec &r, const uint8_t *__restrict__ src, size_t stride,
                                              const int32_t *__restrict__ xs, const int32_t *__restrict__ ys, int dy,
                                              int dx, uint8_t *__restrict__ o) {
    const int h = r.h, w = r.w;
    const int sx = xs[dx], sy0 = ys[dy];
    const int32_t *a = xs + r.ow + (size_t)dx * KS;
    const int32_t *b = ys + r.oh + (size_t)dy * KS;
    if (KS == 2) {
        int32_t hv[2][3];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint8_t *S = src + (size_t)clampi(sy0 + k, 0, h - 1) * stride;
            const int p0 = clampi(sx, 0, w - 1) * 3, p1 = clampi(sx + 1, 0, w - 1) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++)
                hv[k][c] = dx < r.xmax ? S[p0 + c] * a[0] + S[p1 + c] * a[1] : S[p0 + c] * 2048;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            int v;
            if (dx * 3 + c < r.x_vec) {
                const int s0 = clampi(hv[0][c] >> 4, -32768, 32767), s1 = clampi(hv[1][c] >> 4, -32768, 32767);
                int t = ((s0 * b[0]) >> 16) + ((s1 * b[1]) >> 16);
                t = clampi(t, -32768, 32767);
                v = sat8((t + 2) >> 2);
            } else {
                v = sat8((hv[0][c] * b[0] + hv[1][c] * b[1] + (1 << 21)) >> 22);
            }
            o[c] = (uint8_t)v;
        }
    } else {
        int px[8], av[8];
#pragma unroll
        for (int j = 0; j < 8; j++) px[j] = clampi(sx - 3 + j, 0, w - 1) * 3, av[j] = a[j];
        uint32_t s[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint8_t *S = src + (size_t)clampi(sy0 - 3 + k, 0, h - 1) * stride;
            const uint32_t bk = (uint32_t)b[k];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                int32_t v = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) v += S[px[j] + c] * av[j];
                s[c] += (uint32_t)v * bk;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = (uint8_t)sat8(((int32_t)s[c] + (1 << 21)) >> 22);
    }
}

__global__ __launch_bounds__(CT) void k_cv_images_generic(const CvImgRec *__restrict__ recs,
                                                          const CvImgWork *__restrict__ work,
                                                          const int32_t *__restrict__ tab) {
    const CvImgWork wk = work[blockIdx.x];
    const CvImgRec &r = recs[wk.image];
    const int tx = wk.tile % r.tiles_x, ty = wk.tile / r.tiles_x;
    const int x0 = tx * kCvTileW, nx = min(kCvTileW, r.ow - x0);
    const int y0 = ty * r.tile_h, ny = min(r.tile_h, r.oh - y0);
    const size_t dpitch = (size_t)r.ow * 3;
    const int32_t *__restrict__ xs = tab + r.xt, *__restrict__ ys = tab + r.yt;
    for (int e = threadIdx.x; e < ny * kCvTileW; e += CT) {
        const int y = e / kCvTileW, xx = e - y * kCvTileW;
        if (xx >= nx) continue;
        uint8_t *o = r.dst + (size_t)(y0 + y) * dpitch + (size_t)(x0 + xx) * 3;
        if (r.ks == 2) generic_pixel<2>(r, r.src, (size_t)r.src_stride, xs, ys, y0 + y, x0 + xx, o);
        else generic_pixel<8>(r, r.src, (size_t)r.src_stride, xs, ys, y0 + y, x0 + xx, o);
    }
}

// ---------------------------------------------------------------------------- COPY
__global__ __launch_bounds__(CT) void k_cv_images_copy(const CvImgRec *__restrict__ recs,
                                                       const CvImgWork *__restrict__ work) {
    const CvImgWork wk = work[blockIdx.x];
    const CvImgRec &r = recs[wk.image];
    const int tx = wk.tile % r.tiles_x, ty = wk.tile / r.tiles_x;
    const int x0 = tx * kCvTileW, nb = min(kCvTileW, r.ow - x0) * 3;
    const int y0 = ty * r.tile_h, ny = min(r.tile_h, r.oh - y0);
    const size_t dpitch = (size_t)r.ow * 3, xoff = (size_t)x0 * 3;
    uint8_t *__restrict__ dst = r.dst + (size_t)y0 * dpitch + xoff;
    const uint8_t *__restrict__ src = r.src + (size_t)y0 * (size_t)r.src_stride + xoff;
    for (int e = threadIdx.x; e < ny * ROWB; e += CT) {
        const int y = e / ROWB, b = e - y * ROWB;
        if (b < nb) dst[(size_t)y * dpitch + b] = src[(size_t)y * (size_t)r.src_stride + b];
    }
}

}  // namespace

hipError_t launch_cv_images(int kind, const CvImgRec *recs, const CvImgWork *work, int n_work, const int32_t *tab,
                            hipStream_t s) {
    if (n_work <= 0) return hipSuccess;
    switch (kind) {
    case CvResizePlan::COPY: hipLaunchKernelGGL(k_cv_images_copy, dim3(n_work), dim3(CT), 0, s, recs, work); break;
    case CvResizePlan::AREA_FAST:
        hipLaunchKernelGGL(k_cv_images_area_fast, dim3(n_work), dim3(CT), 0, s, recs, work);
        break;
    case CvResizePlan::AREA: hipLaunchKernelGGL(k_cv_images_area, dim3(n_work), dim3(CT), 0, s, recs, work, tab); break;
    case CvResizePlan::GENERIC:
        hipLaunchKernelGGL(k_cv_images_generic, dim3(n_work), dim3(CT), 0, s, recs, work, tab);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace llfe
