// The arithmetic of the JPEG reconstruction, shared by the kernels of a same-size batch
// (jpeg_recon.hip) and the kernel of a mixed-size batch (jpeg_images.hip): libjpeg-turbo's
// ISLOW inverse DCT as its SIMD code computes it, fancy h2v1 / h2v2 upsampling and the 16-bit
// fixed-point YCbCr -> BGR, bit for bit (tests/test_jpeg_coefs.py pins the restatement).
// Device code only.
#ifndef LLFE_JPEG_RECON_CORE_H
#define LLFE_JPEG_RECON_CORE_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace llfe {
namespace jpeg_core {

constexpr int JT = 256;  // threads per workgroup of every reconstruction kernel
constexpr int kBlocksPerPass = JT / 8;  // eight lanes per 8x8 block

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

// One 8x8 block by eight consecutive lanes; every thread of the workgroup calls this together
// (it holds barriers).  Lane j brings row j of the block's coefficients (raw) and of its
// quantisation table (q), zeros for a block that is not there, and gets the eight samples of
// row j back as two dwords.  The block goes through the lane group's padded LDS tile twice:
// columns out for pass 1 (descale 11), rows out for pass 2 (descale 18, +128, saturated to
// 0..255 as libjpeg-turbo's SIMD IDCT does; its C code wraps through a 1024-entry table
// instead, and the two differ only for samples more than 384 outside 0..255).
// tile: [8][9] ints of this lane group (+1: column reads and row writes hit 32 banks).
__device__ __forceinline__ uint2 idct_block_row(int (*tile)[9], const uint4 raw, const uint4 q, const int j) {
    int v[8], ws[8];
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
    const bool dc_only = ((nz >> (threadIdx.x & 56)) & 0xff) == 0;
#pragma unroll
    for (int k = 0; k < 8; k++) tile[j][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) v[r] = tile[r][j];  // column j
    idct8<11>(v, ws);
    if (dc_only) {
#pragma unroll
        for (int r = 0; r < 8; r++) ws[r] = (int16_t)((unsigned)v[0] << 2);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) tile[r][j] = ws[r];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = tile[j][k];  // row j
    idct8<18>(v, ws);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lo |= (unsigned)clamp8(ws[k] + 128) << (8 * k);
        hi |= (unsigned)clamp8(ws[k + 4] + 128) << (8 * k);
    }
    return make_uint2(lo, hi);
}

// Fancy upsampling of one chroma component for four pixels x0 .. x0 + 3 of one row (x0 a
// multiple of 4): near = the chroma row of the pixels, far = the other row of the h2v2 triangle
// (cy - 1 for an even y, cy + 1 for an odd one, clamped by the caller; unused for h2v1).
// cm, c0, c1, c2 = the chroma columns x0 / 2 - 1 .. x0 / 2 + 2, clamped by the caller to the
// component's real 0 .. width - 1, which reproduces libjpeg's first / last column rules.
// replicate: a component of width <= 2, for which libjpeg-turbo keeps plain replication.
__device__ __forceinline__ int4 upsample4(const uint8_t *near, const uint8_t *far, int cm, int c0, int c1, int c2,
                                          bool v2, bool replicate) {
    if (replicate) return make_int4(near[c0], near[c0], near[c1], near[c1]);
    if (!v2) {  // h2v1: 3:1, biases +1 / +2
        const int a = near[cm], b = near[c0], c = near[c1], e = near[c2];
        return make_int4((3 * b + a + 1) >> 2, (3 * b + c + 2) >> 2, (3 * c + b + 1) >> 2, (3 * c + e + 2) >> 2);
    }
    // h2v2: column sums 3 * near + far, then 3:1 with biases +8 / +7
    const int a = 3 * near[cm] + far[cm], b = 3 * near[c0] + far[c0], c = 3 * near[c1] + far[c1],
              e = 3 * near[c2] + far[c2];
    return make_int4((3 * b + a + 8) >> 4, (3 * b + c + 7) >> 4, (3 * c + b + 8) >> 4, (3 * c + e + 7) >> 4);
}

// jdcolor.c build_ycc_rgb_table / ycc_rgb_convert, SCALEBITS = 16
constexpr int kCrR = 91881, kCbB = 116130, kCrG = 46802, kCbG = 22554, kHalf = 1 << 15;

// four pixels (luma as the four bytes of y4) -> their 12 bytes B, G, R, ... as three
// little-endian dwords
__device__ __forceinline__ uint3 ycc_to_bgr4(const unsigned y4, const int4 cb4, const int4 cr4) {
    const int cb[4] = {cb4.x, cb4.y, cb4.z, cb4.w}, cr[4] = {cr4.x, cr4.y, cr4.z, cr4.w};
    unsigned b[4], g[4], r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int Y = (y4 >> (8 * k)) & 255, u = cb[k] - 128, v = cr[k] - 128;
        b[k] = (unsigned)clamp8(Y + ((kCbB * u + kHalf) >> 16));
        g[k] = (unsigned)clamp8(Y + ((-kCbG * u + kHalf - kCrG * v) >> 16));
        r[k] = (unsigned)clamp8(Y + ((kCrR * v + kHalf) >> 16));
    }
    return make_uint3(b[0] | g[0] << 8 | r[0] << 16 | b[1] << 24, g[1] | r[1] << 8 | b[2] << 16 | g[2] << 24,
                      r[2] | b[3] << 8 | g[3] << 16 | r[3] << 24);
}

// four samples of one row in a dword -> int4
__device__ __forceinline__ int4 bytes4(unsigned v) {
    return make_int4(v & 255, (v >> 8) & 255, (v >> 16) & 255, v >> 24);
}

// the 12 bytes of pixels x0 .. x0 + 3 of a row of width w to o: three dwords when the rows are
// 4-byte aligned (vec) and all four pixels are there, bytes otherwise and at the row's end
__device__ __forceinline__ void store_bgr4(uint8_t *o, const uint3 px, int vec, int x0, int w) {
    if (vec && x0 + 4 <= w) {
        unsigned *o4 = (unsigned *)o;
        o4[0] = px.x;
        o4[1] = px.y;
        o4[2] = px.z;
    } else {
        const int nb = 3 * min(4, w - x0);
#pragma unroll
        for (int k = 0; k < 12; k++)
            if (k < nb) o[k] = (uint8_t)((k < 4 ? px.x : k < 8 ? px.y : px.z) >> (8 * (k & 3)));
    }
}

}  // namespace jpeg_core
}  // namespace llfe
#endif
