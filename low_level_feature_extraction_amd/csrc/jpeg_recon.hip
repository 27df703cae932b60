// The reconstruction half of a JPEG decode on the device: quantised coefficients (staged by
// llfe_jpeg_read_coefs_batch, jpeg_decode.cpp) -> the N x H x W x 3 BGR batch, bit for bit
// what libjpeg-turbo writes at OpenCV's settings for cv2.imdecode(buf, IMREAD_COLOR)
// (app/services/analyze/utils.py:108-109, image_processor.py:208-211): ISLOW inverse DCT,
// fancy upsampling, JCS_EXT_BGR.
//
// Two kernels per chunk of images.
//   k_jpeg_idct:  eight lanes per 8x8 block.  Lane j loads row j of the block (16 bytes; a
//                 wave reads eight blocks = 1 KiB in one instruction) and row j of the
//                 quantisation table, dequantises, and the block goes through a padded
//                 LDS tile twice: columns out for pass 1 (descale 11), rows out for pass 2
//                 (descale 18, +128, saturated to 0..255 as libjpeg-turbo's SIMD IDCT does;
//                 its C code wraps through a 1024-entry table instead, and the two differ
//                 only for samples more than 384 outside 0..255, tests/test_jpeg_coefs.py).
//                 Lane j stores 8 samples of row j into the
//                 component's u8 plane, which is padded to whole blocks so no store needs a
//                 bound.  32 blocks per workgroup, 9.2 KiB of LDS.
//   k_jpeg_color: four pixels of one row per lane: 4 luma bytes in one load, the chroma
//                 neighbourhood of two columns (clamped at the component's real edges,
//                 which reproduces libjpeg's first / last column and row rules exactly),
//                 h2v1 or h2v2 triangle filter or replication, the 16-bit fixed-point
//                 YCbCr -> BGR, 12 bytes out (three dwords when the rows are 4-byte aligned).
// The sampling class of an image is uniform over a workgroup (blockIdx.z = image).
//
// Every index derives from a descriptor that validate_jpeg_descs() accepted on the host:
// offsets inside the slot, block grids that cover the image, planes inside the workspace.
#include <algorithm>

#include "jpeg_desc_check.h"
#include "llfe_internal.h"

namespace llfe {
namespace {

constexpr int JT = 256;           // threads per workgroup, both kernels
constexpr int kBlocksPerWg = JT / 8;

// jidctint.c: 13-bit constants, CONST_BITS = 13, PASS1_BITS = 2
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270,
              F_0_899976223 = 7373, F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137,
              F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;

// One 8-point pass of jpeg_idct_islow as libjpeg-turbo's SIMD code computes it (the code
// OpenCV's decode runs on x86): the sums in0 +- in4, in7 + in3 and in5 + in1 are 16-bit adds,
// everything else 32-bit and wrapping (hence unsigned here), and the descaled result,
// (x + 2^(SHIFT-1)) >> SHIFT, is packed with saturation to 16 bits.  For every coefficient an
// encoder of 8-bit samples emits nothing wraps and this is the C code's arithmetic; hand-made
// tables beyond that are decoded as the library decodes them (tests/test_jpeg_coefs.py).
__device__ __forceinline__ unsigned s16(unsigned v) { return (unsigned)(int)(int16_t)v; }
__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

template <int SHIFT>
__device__ __forceinline__ void idct8(const int (&x)[8], int (&out)[8]) {
    typedef unsigned U;
    const U in0 = (U)x[0], in1 = (U)x[1], in2 = (U)x[2], in3 = (U)x[3], in4 = (U)x[4], in5 = (U)x[5], in6 = (U)x[6],
            in7 = (U)x[7];
    U z1 = (in2 + in6) * (U)F_0_541196100;
    U tmp2 = z1 - in6 * (U)F_1_847759065;
    U tmp3 = z1 + in2 * (U)F_0_765366865;
    U tmp0 = s16(in0 + in4) << 13;
    U tmp1 = s16(in0 - in4) << 13;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in7;
    tmp1 = in5;
    tmp2 = in3;
    tmp3 = in1;
    z1 = tmp0 + tmp3;
    U z2 = tmp1 + tmp2;
    U z3 = s16(tmp0 + tmp2);
    U z4 = s16(tmp1 + tmp3);
    const U z5 = (z3 + z4) * (U)F_1_175875602;
    tmp0 *= (U)F_0_298631336;
    tmp1 *= (U)F_2_053119869;
    tmp2 *= (U)F_3_072711026;
    tmp3 *= (U)F_1_501321110;
    z1 *= (U)-F_0_899976223;
    z2 *= (U)-F_2_562915447;
    z3 = z3 * (U)-F_1_961570560 + z5;
    z4 = z4 * (U)-F_0_390180644 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr U R = 1u << (SHIFT - 1);
    out[0] = sat16((int)(tmp10 + tmp3 + R) >> SHIFT);
    out[7] = sat16((int)(tmp10 - tmp3 + R) >> SHIFT);
    out[1] = sat16((int)(tmp11 + tmp2 + R) >> SHIFT);
    out[6] = sat16((int)(tmp11 - tmp2 + R) >> SHIFT);
    out[2] = sat16((int)(tmp12 + tmp1 + R) >> SHIFT);
    out[5] = sat16((int)(tmp12 - tmp1 + R) >> SHIFT);
    out[3] = sat16((int)(tmp13 + tmp0 + R) >> SHIFT);
    out[4] = sat16((int)(tmp13 - tmp0 + R) >> SHIFT);
}

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__global__ __launch_bounds__(JT) void k_jpeg_idct(const uint8_t *__restrict__ coefs, int64_t slot_stride,
                                                  const llfe_jpeg_desc *__restrict__ descs,
                                                  uint8_t *__restrict__ planes, int64_t plane_stride) {
    __shared__ int tile[kBlocksPerWg][8][9];  // (+1: column reads and row writes hit 32 banks)
    const int img = blockIdx.z, c = blockIdx.y;
    const llfe_jpeg_desc &d = descs[img];
    if (c >= d.n_comp) return;  // (whole workgroup: n_comp 0 = an image staged elsewhere)
    const int bw = d.comp[c].blocks_w;
    const int nblk = bw * d.comp[c].blocks_h;
    if ((int)blockIdx.x * kBlocksPerWg >= nblk) return;  // (whole workgroup)
    const int g = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int blk = (int)blockIdx.x * kBlocksPerWg + g;
    const bool act = blk < nblk;
    const uint8_t *slot = coefs + (int64_t)img * slot_stride;
    int v[8], ws[8];
    bool dc_only;
    {
        uint4 raw = make_uint4(0, 0, 0, 0), q = raw;
        if (act) {
            raw = *(const uint4 *)(slot + d.comp[c].coef_offset + (int64_t)blk * 128 + j * 16);
            q = *(const uint4 *)(slot + d.comp[c].quant_offset + j * 16);
        }
        // DEQUANTIZE: a 16-bit product (pmullw)
        const unsigned rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[2 * k] = (int16_t)((rw[k] & 0xffff) * (qw[k] & 0xffff));
            v[2 * k + 1] = (int16_t)((rw[k] >> 16) * (qw[k] >> 16));
        }
        // rows 1..7 of the block's coefficients all zero: the library's pass 1 is then its
        // shortcut, each column = its dequantised DC << 2 in 16 bits
        const unsigned long long nz = __ballot(j != 0 && (raw.x | raw.y | raw.z | raw.w) != 0);
        dc_only = ((nz >> (threadIdx.x & 56)) & 0xff) == 0;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) tile[g][j][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) v[r] = tile[g][r][j];  // column j
    idct8<11>(v, ws);
    if (dc_only) {
#pragma unroll
        for (int r = 0; r < 8; r++) ws[r] = (int16_t)((unsigned)v[0] << 2);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) tile[g][r][j] = ws[r];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = tile[g][j][k];  // row j
    idct8<18>(v, ws);
    if (!act) return;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lo |= (unsigned)clamp8(ws[k] + 128) << (8 * k);
        hi |= (unsigned)clamp8(ws[k + 4] + 128) << (8 * k);
    }
    const int by = blk / bw, bx = blk - by * bw;
    uint8_t *plane = planes + (int64_t)img * plane_stride + plane_offset(d, c);
    *(uint2 *)(plane + ((int64_t)by * 8 + j) * ((int64_t)bw * 8) + bx * 8) = make_uint2(lo, hi);
}

// jdcolor.c build_ycc_rgb_table / ycc_rgb_convert, SCALEBITS = 16
constexpr int kCrR = 91881, kCbB = 116130, kCrG = 46802, kCbG = 22554, kHalf = 1 << 15;

__global__ __launch_bounds__(JT) void k_jpeg_color(const llfe_jpeg_desc *__restrict__ descs,
                                                   const uint8_t *__restrict__ planes, int64_t plane_stride, int h,
                                                   int w, uint8_t *__restrict__ out, int vec) {
    const int img = blockIdx.z;
    const llfe_jpeg_desc &d = descs[img];
    if (d.n_comp == 0) return;
    const int x0 = ((int)blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= w || y >= h) return;
    const uint8_t *p0 = planes + (int64_t)img * plane_stride;
    const unsigned y4 = *(const unsigned *)(p0 + (int64_t)y * (d.comp[0].blocks_w * 8) + x0);
    int Y[4], cb[4], cr[4];
#pragma unroll
    for (int k = 0; k < 4; k++) Y[k] = (y4 >> (8 * k)) & 255;
    const int cls = d.sampling;
    if (cls == LLFE_JPEG_GRAY) {
#pragma unroll
        for (int k = 0; k < 4; k++) cb[k] = cr[k] = 128;
    } else {
        const int pitch = d.comp[1].blocks_w * 8;  // (validated: both chroma components alike)
        const uint8_t *p1 = p0 + plane_offset(d, 1), *p2 = p0 + plane_offset(d, 2);
        if (cls == LLFE_JPEG_444) {
            const unsigned b4 = *(const unsigned *)(p1 + (int64_t)y * pitch + x0);
            const unsigned r4 = *(const unsigned *)(p2 + (int64_t)y * pitch + x0);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                cb[k] = (b4 >> (8 * k)) & 255;
                cr[k] = (r4 >> (8 * k)) & 255;
            }
        } else {
            const int dw = d.comp[1].width, dh = d.comp[1].height;
            const bool v2 = cls == LLFE_JPEG_420;
            const int cy = v2 ? y >> 1 : y;
            const int c0 = x0 >> 1;
            const int c1 = min(c0 + 1, dw - 1);
            const uint8_t *pl[2] = {p1, p2};
            int *dst[2] = {cb, cr};
            if (dw <= 2) {  // libjpeg-turbo keeps plain replication for such a component
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const uint8_t *row = pl[t] + (int64_t)cy * pitch;
                    dst[t][0] = dst[t][1] = row[c0];
                    dst[t][2] = dst[t][3] = row[c1];
                }
            } else {
                const int cm = max(c0 - 1, 0), c2 = min(c0 + 2, dw - 1);
                if (!v2) {  // h2v1: 3:1, biases +1 / +2
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const uint8_t *row = pl[t] + (int64_t)cy * pitch;
                        const int a = row[cm], b = row[c0], c = row[c1], e = row[c2];
                        dst[t][0] = (3 * b + a + 1) >> 2;
                        dst[t][1] = (3 * b + c + 2) >> 2;
                        dst[t][2] = (3 * c + b + 1) >> 2;
                        dst[t][3] = (3 * c + e + 2) >> 2;
                    }
                } else {  // h2v2: column sums 3 * near + far, then 3:1 with biases +8 / +7
                    const int fy = (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const uint8_t *near = pl[t] + (int64_t)cy * pitch, *far = pl[t] + (int64_t)fy * pitch;
                        const int a = 3 * near[cm] + far[cm], b = 3 * near[c0] + far[c0],
                                  c = 3 * near[c1] + far[c1], e = 3 * near[c2] + far[c2];
                        dst[t][0] = (3 * b + a + 8) >> 4;
                        dst[t][1] = (3 * b + c + 7) >> 4;
                        dst[t][2] = (3 * c + b + 8) >> 4;
                        dst[t][3] = (3 * c + e + 7) >> 4;
                    }
                }
            }
        }
    }
    uint8_t px[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int u = cb[k] - 128, v = cr[k] - 128;
        px[3 * k] = (uint8_t)clamp8(Y[k] + ((kCbB * u + kHalf) >> 16));
        px[3 * k + 1] = (uint8_t)clamp8(Y[k] + ((-kCbG * u + kHalf - kCrG * v) >> 16));
        px[3 * k + 2] = (uint8_t)clamp8(Y[k] + ((kCrR * v + kHalf) >> 16));
    }
    uint8_t *o = out + ((int64_t)img * h * w + (int64_t)y * w + x0) * 3;
    if (vec && x0 + 4 <= w) {
        unsigned wd[3];
#pragma unroll
        for (int k = 0; k < 3; k++)
            wd[k] = px[4 * k] | (unsigned)px[4 * k + 1] << 8 | (unsigned)px[4 * k + 2] << 16 | (unsigned)px[4 * k + 3] << 24;
        unsigned *o4 = (unsigned *)o;
        o4[0] = wd[0];
        o4[1] = wd[1];
        o4[2] = wd[2];
    } else {
        const int nb = 3 * min(4, w - x0);
        for (int k = 0; k < nb; k++) o[k] = px[k];
    }
}

}  // namespace

bool validate_jpeg_descs(const llfe_jpeg_desc *descs, int n, int h, int w, int64_t slot_stride,
                         int64_t *plane_stride, int *max_blocks) {
    return check_jpeg_descs(descs, n, h, w, slot_stride, plane_stride, max_blocks);  // jpeg_desc_check.h
}

hipError_t launch_jpeg_reconstruct(const uint8_t *coefs, int64_t slot_stride, const llfe_jpeg_desc *d_descs, int n,
                                   int h, int w, int max_blocks, uint8_t *planes, int64_t plane_stride, uint8_t *out,
                                   hipStream_t s, int stage) {
    if (n <= 0 || max_blocks <= 0) return hipSuccess;
    if (stage == 0) {
        const dim3 grid((unsigned)((max_blocks + kBlocksPerWg - 1) / kBlocksPerWg), 3, (unsigned)n);
        hipLaunchKernelGGL(k_jpeg_idct, grid, dim3(JT), 0, s, coefs, slot_stride, d_descs, planes, plane_stride);
    } else {
        const int vec = (w % 4 == 0 && ((uintptr_t)out & 3) == 0) ? 1 : 0;
        const dim3 grid((unsigned)((w + 255) / 256), (unsigned)((h + 3) / 4), (unsigned)n);
        hipLaunchKernelGGL(k_jpeg_color, grid, dim3(JT), 0, s, d_descs, planes, plane_stride, h, w, out, vec);
    }
    return hipGetLastError();
}

}  // namespace llfe
