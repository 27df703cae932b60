// Image.thumbnail((max_w, max_h), LANCZOS) of a batch of images of any sizes
// (llfe_thumbnail_pil_images): resize.hip's arithmetic, ragged.
//
// The host builds one record per image (ThumbRec: pointers, strides, sizes, the offsets of its
// plan's bounds and coefficients in one int32 table) and one work table of (image, tile)
// entries; a workgroup takes one entry.  Nothing is shared between workgroups and nothing is
// accumulated across them: no atomics.  Every index below derives from a record whose bounds
// the host checked against the image sizes and the LDS budget before the launch.
//
//   k_thumb_reduce   Pillow's reduce() pre-pass (k_reduce) over the images whose factor
//                    exceeds 1, a tile of kThumbReduceBytes row bytes x kThumbReduceRows rows
//   k_thumb_lanczos  an output tile of kThumbTileW pixels x tile_h rows.  With both passes the
//                    horizontal pass of the source rows the tile needs goes to LDS as u8
//                    (a lane per pixel; clip8 after the 22-bit sum: exactly Pillow's u8
//                    intermediate) and the vertical pass runs from LDS to dst, lanes along row
//                    bytes, four to a lane; an image that needs one pass writes it straight to
//                    dst; one that fits is copied.
// A ragged two-pass form with an HBM intermediate measured 2.2 times slower.
#include "llfe_internal.h"

namespace llfe {
namespace {

constexpr int PREC = 22;
constexpr int TT = 256;
constexpr int ROWB = kThumbTileW * 3;  // bytes of a tile row

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= PREC;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(TT) void k_thumb_reduce(const ThumbRec *__restrict__ recs,
                                                     const ThumbWork *__restrict__ work) {
    const ThumbWork wk = work[blockIdx.x];
    const ThumbRec &r = recs[wk.image];
    const int tx = wk.tile % r.rtiles_x, ty = wk.tile / r.rtiles_x;
    const long long rowlen = (long long)r.rw * 3;
    const long long i = (long long)tx * kThumbReduceBytes + threadIdx.x;
    if (i >= rowlen) return;
    const int xx = (int)(i / 3), c = (int)(i - (long long)xx * 3);
    const int fx = r.fx, fy = r.fy;
    const int xa = xx * fx, xb = min(r.w, xa + fx);
    const uint8_t *__restrict__ src = r.rsrc;
    const size_t stride = (size_t)r.rsrc_stride;
    const int y_end = min(r.rh, (ty + 1) * kThumbReduceRows);
    for (int yy = ty * kThumbReduceRows; yy < y_end; yy++) {
        const int ya = yy * fy, yb = min(r.h, ya + fy);
        const uint32_t n = (uint32_t)((yb - ya) * (xb - xa));
        const uint32_t mult = (uint32_t)(4294967296.0f / (float)(256u * n));
        uint32_t ss = n / 2;
        for (int y = ya; y < yb; y++)
            for (int x = xa; x < xb; x++) ss += src[(size_t)y * stride + (size_t)x * 3 + c];
        r.red[(size_t)yy * (size_t)rowlen + (size_t)i] = (uint8_t)((ss * mult) >> 24);
    }
}

// horizontal pass of one pixel: output pixel x0 + xx of the tile from a source row, the three
// channels sharing each coefficient
__device__ __forceinline__ void hpass(const uint8_t *__restrict__ row, const int32_t *s_bh, const int32_t *s_kh,
                                      int ksh, int xx, uint8_t *out) {
    const int xmin = s_bh[2 * xx], xmax = s_bh[2 * xx + 1];
    const int32_t *k = s_kh + xx * ksh;
    const uint8_t *p = row + (size_t)xmin * 3;
    int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < xmax; x++, p += 3) {
        const int kx = k[x];
        s0 += (int)p[0] * kx;
        s1 += (int)p[1] * kx;
        s2 += (int)p[2] * kx;
    }
    out[0] = clip8(s0), out[1] = clip8(s1), out[2] = clip8(s2);
}

__global__ __launch_bounds__(TT) void k_thumb_lanczos(const ThumbRec *__restrict__ recs,
                                                      const ThumbWork *__restrict__ work,
                                                      const int32_t *__restrict__ tab) {
    __shared__ int32_t s_kh[kThumbTileW * kThumbMaxK];
    __shared__ int32_t s_bh[kThumbTileW * 2];
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kThumbLdsRows * ROWB];
    const ThumbWork wk = work[blockIdx.x];
    const ThumbRec &r = recs[wk.image];
    const int tid = threadIdx.x;
    const int tx = wk.tile % r.tiles_x, ty = wk.tile / r.tiles_x;
    const int x0 = tx * kThumbTileW, nb = min(kThumbTileW, r.ow - x0) * 3;
    const int y0 = ty * r.tile_h, ny = min(r.tile_h, r.oh - y0);
    const size_t dpitch = (size_t)r.ow * 3, xoff = (size_t)x0 * 3;
    uint8_t *__restrict__ dst = r.dst + (size_t)y0 * dpitch + xoff;
    const uint8_t *__restrict__ src = r.src;
    const size_t stride = (size_t)r.src_stride;
    const int mode = r.mode;

    if (mode == kThumbCopy) {
        for (int e = tid; e < ny * ROWB; e += TT) {
            const int y = e / ROWB, b = e - y * ROWB;
            if (b < nb) dst[(size_t)y * dpitch + b] = src[(size_t)(y0 + y) * stride + xoff + b];
        }
        return;
    }
    const int ksv = r.ksv, yfirst = r.yfirst;
    const int32_t *__restrict__ bv = tab + r.bv;
    const int32_t *__restrict__ kv = tab + r.kv;
    if (mode == kThumbV) {
        for (int e = tid; e < ny * ROWB; e += TT) {
            const int y = e / ROWB, b = e - y * ROWB;
            if (b >= nb) continue;
            const int yy = y0 + y;
            const int ymin = bv[2 * yy] + yfirst, ymax = bv[2 * yy + 1];
            const int32_t *k = kv + (size_t)yy * ksv;
            const uint8_t *col = src + (size_t)ymin * stride + xoff + b;
            int ss = 1 << (PREC - 1);
            for (int t = 0; t < ymax; t++) ss += (int)col[(size_t)t * stride] * k[t];
            dst[(size_t)y * dpitch + b] = clip8(ss);
        }
        return;
    }
    // the tile's horizontal bounds and coefficients
    const int ksh = r.ksh, nx = nb / 3;
    for (int e = tid; e < nx * ksh; e += TT) s_kh[e] = tab[(size_t)r.kh + (size_t)x0 * ksh + e];
    for (int e = tid; e < nx * 2; e += TT) s_bh[e] = tab[(size_t)r.bh + 2 * (size_t)x0 + e];
    __syncthreads();
    if (mode == kThumbH) {
        for (int e = tid; e < ny * kThumbTileW; e += TT) {
            const int y = e / kThumbTileW, xx = e - y * kThumbTileW;
            if (xx < nx)
                hpass(src + (size_t)(yfirst + y0 + y) * stride, s_bh, s_kh, ksh, xx, dst + (size_t)y * dpitch + xx * 3);
        }
        return;
    }
    // both passes: source rows [yfirst + r0, yfirst + r1) through the horizontal pass into LDS
    const int r0 = bv[2 * y0], r1 = bv[2 * (y0 + ny - 1)] + bv[2 * (y0 + ny - 1) + 1];
    const int nrows = r1 - r0;
    for (int e = tid; e < nrows * kThumbTileW; e += TT) {
        const int rr = e / kThumbTileW, xx = e - rr * kThumbTileW;
        if (xx < nx) hpass(src + (size_t)(yfirst + r0 + rr) * stride, s_bh, s_kh, ksh, xx, s_rows + rr * ROWB + xx * 3);
    }
    __syncthreads();
    // vertical pass: a lane takes four consecutive row bytes (one LDS word per tap)
    constexpr int ROWW = ROWB / 4;
    for (int e = tid; e < ny * ROWW; e += TT) {
        const int y = e / ROWW, b = (e - y * ROWW) * 4;
        if (b >= nb) continue;
        const int yy = y0 + y;
        const int ymin = bv[2 * yy] - r0, ymax = bv[2 * yy + 1];
        const int32_t *k = kv + (size_t)yy * ksv;
        const uint32_t *col = (const uint32_t *)(s_rows + ymin * ROWB + b);
        int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0, s3 = s0;
        for (int t = 0; t < ymax; t++) {
            const uint32_t v = col[t * ROWW];
            const int kt = k[t];
            s0 += (int)(v & 255u) * kt;
            s1 += (int)((v >> 8) & 255u) * kt;
            s2 += (int)((v >> 16) & 255u) * kt;
            s3 += (int)(v >> 24) * kt;
        }
        uint8_t *o = dst + (size_t)y * dpitch + b;
        o[0] = clip8(s0);
        if (b + 1 < nb) o[1] = clip8(s1);
        if (b + 2 < nb) o[2] = clip8(s2);
        if (b + 3 < nb) o[3] = clip8(s3);
    }
}

}  // namespace

hipError_t launch_thumb_reduce(const ThumbRec *recs, const ThumbWork *work, int n_work, hipStream_t s) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_thumb_reduce, dim3(n_work), dim3(TT), 0, s, recs, work);
    return hipGetLastError();
}

hipError_t launch_thumb_lanczos(const ThumbRec *recs, const ThumbWork *work, int n_work, const int32_t *tab,
                                hipStream_t s) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_thumb_lanczos, dim3(n_work), dim3(TT), 0, s, recs, work, tab);
    return hipGetLastError();
}

}  // namespace llfe
