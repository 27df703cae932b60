// FontDetector.preprocess_image (app/services/analyze/font_detector.py:17-37) straight to
// the bit rows the contour pass reads: BGR -> gray -> adaptiveThreshold(GAUSSIAN_C,
// THRESH_BINARY_INV, 11, 2) -> n x h x ceil(w / 64) u64, bit x & 63 of word x >> 6 = pixel x,
// every bit at x >= w zero.  One pass, no u8 mask in between: bit for bit what
// k_font_pack(k_font_binary(bgr)) (stencil.hip's font mode + font.hip) produces.
//
//   gray  = (1868 B + 9617 G + 4899 R + 8192) >> 14
//   mean  = clamp(rint(CV_32F Gauss11 x Gauss11 over gray, BORDER_REPLICATE), 0, 255) with
//           OpenCV's evaluation order (stencil.hip steps 6-7): the row pass one fma chain
//           left -> right from 0 over taps 0..10, the column pass centre x w5 then the
//           symmetric pairs (a + b) . w inner -> outer
//   bit   = gray - mean <= -2
//
// Layout (row streaming, in the manner of stencil_stream.hip).  One wave owns a strip of
// 256 columns -- 64 lanes x 4 pixels, one packed dword of gray per lane -- and marches down a
// segment of rows.  The strip is 4 whole output words, so every word is written by exactly
// one wave (no atomics, no zeroed output); the 5-column halo on each side comes from two
// extra dwords per side that lanes 0..3 load and convert, handed to lanes 0 / 63 through
// v_readlane.  All other horizontal neighbours come by DPP wave shifts.  The 11 row-pass rows
// the column pass needs sit in a register ring of 12 (the row loop is unrolled 12 times, so a
// ring slot is a fixed register), the gray rows in a ring of 6, the input rows two steps
// ahead in a ring of 3.  No LDS, no workgroup barriers.  A segment recomputes 10 rows of row
// pass (5 above, 5 below).
//
// REPLICATE borders are clamped loads: rows by clamping the row index; columns by loading
// the dword column clamped into the image and splatting its first / last byte (aligned
// rows: w % 4 == 0 and a 4-byte aligned image), or pixel by pixel with clamped columns
// (any other image).  Every load is inside the image.
#include <algorithm>

#include "llfe_internal.h"

namespace llfe {
namespace {

__device__ __constant__ constexpr float kGauss11[11] = {LLFE_GAUSS11_F32};

constexpr int kStripW = 256;  // 64 lanes x 4 columns = 4 output words
constexpr int kSegRows = 216; // rows per segment (balanced over the image's height)
constexpr int kWavesPerBlock = 4;

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 U(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 255u; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// DPP wave shifts: from_left(v) in lane L is v of lane L - 1, from_right(v) of lane L + 1
// (the lanes shifted in at the wave's ends read 0: lanes 0 / 63 take the halo instead)
__device__ __forceinline__ uint32_t from_left(uint32_t v) { return __builtin_amdgcn_mov_dpp(v, 0x138, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t from_right(uint32_t v) { return __builtin_amdgcn_mov_dpp(v, 0x130, 0xf, 0xf, true); }

struct Raw {
    uint32_t a, b, c;
};

// 4 BGR pixels of one row at columns xc .. xc + 3: one 12-byte load (aligned rows; the
// caller clamps xc into [0, W - 4]), else 12 byte loads from the columns clamped into the row
__device__ __forceinline__ Raw load_px(const uint8_t *__restrict__ row, int W, int xc, bool vec) {
    Raw r;
    if (vec) {
        const uint32_t *p = (const uint32_t *)(row + (uint32_t)(xc * 3));
        r.a = p[0];
        r.b = p[1];
        r.c = p[2];
    } else {
        uint32_t v[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint8_t *q = row + (uint32_t)(clampi(xc + j, 0, W - 1) * 3);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int k = 3 * j + c;
                v[k >> 2] |= (uint32_t)q[c] << (8 * (k & 3));
            }
        }
        r.a = v[0];
        r.b = v[1];
        r.c = v[2];
    }
    return r;
}

// Y = (B*1868 + G*9617 + R*4899 + 2^13) >> 14 for the 4 pixels -> packed u8x4
__device__ __forceinline__ uint32_t gray4(Raw r) {
    const u16x2 bg0 = U(__builtin_amdgcn_perm(0u, r.a, 0x0c010c00u));
    const u16x2 bg1 = U(__builtin_amdgcn_perm(r.b, r.a, 0x0c040c03u));
    const u16x2 bg2 = U(__builtin_amdgcn_perm(0u, r.b, 0x0c030c02u));
    const u16x2 bg3 = U(__builtin_amdgcn_perm(0u, r.c, 0x0c020c01u));
    const u16x2 wbg = {1868, 9617};
    const uint32_t y0 = __builtin_amdgcn_udot2(bg0, wbg, byte_of(r.a, 2) * 4899u + 8192u, false) >> 14;
    const uint32_t y1 = __builtin_amdgcn_udot2(bg1, wbg, byte_of(r.b, 1) * 4899u + 8192u, false) >> 14;
    const uint32_t y2 = __builtin_amdgcn_udot2(bg2, wbg, byte_of(r.c, 0) * 4899u + 8192u, false) >> 14;
    const uint32_t y3 = __builtin_amdgcn_udot2(bg3, wbg, byte_of(r.c, 3) * 4899u + 8192u, false) >> 14;
    return y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
}

// CV_32F Gauss11 row pass (s = 0; s = fma(x[k - 5], k[k], s) left -> right) of the lane's 4
// columns c0 .. c0 + 3 of one gray row: g is the lane's dword, l1 / l2 the dwords one / two
// to the left, r1 / r2 to the right.  Packed FP32: columns c0 and c2 share one chain of
// v_pk_fma_f32, c1 and c3 the other -- each half is its own exact fma chain, in order
__device__ __forceinline__ void rowpass4(uint32_t l2, uint32_t l1, uint32_t g, uint32_t r1, uint32_t r2,
                                         f32x2 &o02, f32x2 &o13) {
    float x[14];  // index 0 = column c0 - 5
    x[0] = (float)byte_of(l2, 3);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        x[1 + i] = (float)byte_of(l1, i);
        x[5 + i] = (float)byte_of(g, i);
        x[9 + i] = (float)byte_of(r1, i);
    }
    x[13] = (float)byte_of(r2, 0);
    f32x2 a = {0.0f, 0.0f}, b = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const f32x2 w = {kGauss11[k], kGauss11[k]};
        a = __builtin_elementwise_fma(f32x2{x[k], x[k + 2]}, w, a);
        b = __builtin_elementwise_fma(f32x2{x[k + 1], x[k + 3]}, w, b);
    }
    o02 = a;
    o13 = b;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_font_bits(const uint8_t *__restrict__ bgr,
                                                                   const uint64_t *__restrict__ img_tab, int H, int W,
                                                                   int strips, int segs, int seg_rows,
                                                                   int total_waves, int wpr,
                                                                   uint64_t *__restrict__ bits) {
    // wave-uniform work item: strip x segment of one image
    const int wid = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wid >= total_waves) return;  // whole wave leaves
    const int lane = threadIdx.x & 63;
    const int strip = wid % strips;
    const int rest = wid / strips;
    const int seg = rest % segs;
    const int img_i = rest / segs;
    const uint8_t *img = img_tab ? (const uint8_t *)img_tab[img_i] : bgr + (size_t)img_i * H * W * 3;
    uint32_t *const out = (uint32_t *)(bits + (size_t)img_i * H * wpr);  // two dwords per word
    const int ya = seg * seg_rows, yb = min(H, ya + seg_rows);
    const int x0 = strip * kStripW, x = x0 + 4 * lane;  // the lane's first column
    const bool vec = (((uintptr_t)img & 3) == 0) && (W & 3) == 0;  // wave-uniform
    // the wave reaches past the image's left / right border: splat fix-ups below
    const bool edge = x0 == 0 || x0 + kStripW + 8 > W;
    // halo dwords: lanes 0, 1 hold columns x0 - 8 .. x0 - 1, lanes 2, 3 x0 + 256 .. x0 + 263
    const bool halo_lane = lane < 4;
    const int hx = lane < 2 ? x0 - 8 + 4 * lane : x0 + kStripW + 4 * (lane - 2);
    // aligned rows: the dword column clamped into the image (W >= 4 there); the bytes of a
    // dword wholly outside are then the splat of its byte nearest the image
    const int xl = vec ? min(x, W - 4) : x, hxl = vec ? clampi(hx, 0, W - 4) : hx;
    const bool store_lane = (lane & 7) == 0 && (x >> 6) < wpr;

    constexpr int kU = 12;
    const int t0 = ya - 5, t_end = yb + 5, ts = t0 - 2;
    const int tb0 = ts >= 0 ? ts - ts % kU : -(((-ts) + kU - 1) / kU) * kU;  // floor to a multiple of kU
    Raw Q[3], Qh[3];
    uint32_t G[6];
    f32x2 ra[kU], rb[kU];
#pragma unroll
    for (int k = 0; k < 3; k++) Q[k] = Qh[k] = Raw{0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 6; k++) G[k] = 0;
#pragma unroll
    for (int k = 0; k < kU; k++) ra[k] = rb[k] = f32x2{0.0f, 0.0f};

    // Row steps t = ya - 5 .. yb + 4 (virtual rows; row clamp(t, 0, H - 1) of the image):
    //   input   Q / Qh[3]: row t + 2 issued at step t, slot (t + 2) % 3
    //   gray    G[6]:      row t, slot t % 6 (the threshold reads row t - 5)
    //   row pass ra / rb[12]: row t, slot t % 12 (the column pass reads rows t - 10 .. t)
    // and from t = ya + 5 on, output row t - 5.
    for (int tb = tb0; tb < t_end; tb += kU) {
#pragma unroll
        for (int k = 0; k < kU; k++) {
            const int t = tb + k;
            if (t >= ts && t < t_end) {  // (no break: the loop must unroll so ring slots are registers)
                if (t + 2 < t_end) {
                    const uint8_t *row = img + (size_t)clampi(t + 2, 0, H - 1) * W * 3;  // 64-bit: may pass 2^31
                    Q[(k + 2) % 3] = load_px(row, W, xl, vec);
                    if (halo_lane) Qh[(k + 2) % 3] = load_px(row, W, hxl, vec);
                }
                if (t >= t0) {
                    uint32_t g = gray4(Q[k % 3]), hg = gray4(Qh[k % 3]);
                    if (edge) {  // REPLICATE beyond columns 0 / W - 1
                        if (x >= W) g = (g >> 24) * 0x01010101u;
                        if (hx < 0) hg = (hg & 255u) * 0x01010101u;
                        if (hx >= W) hg = (hg >> 24) * 0x01010101u;
                    }
                    G[k % 6] = g;
                    const uint32_t h0 = __builtin_amdgcn_readlane(hg, 0), h1 = __builtin_amdgcn_readlane(hg, 1);
                    const uint32_t h2 = __builtin_amdgcn_readlane(hg, 2), h3 = __builtin_amdgcn_readlane(hg, 3);
                    uint32_t l1 = from_left(g);
                    if (lane == 0) l1 = h1;
                    uint32_t l2 = from_left(l1);
                    if (lane == 0) l2 = h0;
                    uint32_t r1 = from_right(g);
                    if (lane == 63) r1 = h2;
                    uint32_t r2 = from_right(r1);
                    if (lane == 63) r2 = h3;
                    rowpass4(l2, l1, g, r1, r2, ra[k], rb[k]);
                    const int yo = t - 5;
                    if (yo >= ya) {  // (yo < yb: t < yb + 5)
                        const int kc = (k + kU - 5) % kU;
                        const f32x2 w5 = {kGauss11[5], kGauss11[5]};
                        f32x2 pa[5], pb[5];
#pragma unroll
                        for (int d = 1; d <= 5; d++) {
                            const int kp = (kc + d) % kU, kq = (kc + kU - d) % kU;
                            pa[d - 1] = ra[kp] + ra[kq];
                            pb[d - 1] = rb[kp] + rb[kq];
                        }
                        f32x2 s02 = ra[kc] * w5, s13 = rb[kc] * w5;
#pragma unroll
                        for (int d = 1; d <= 5; d++) {
                            const f32x2 wd = {kGauss11[5 + d], kGauss11[5 + d]};
                            s02 = __builtin_elementwise_fma(pa[d - 1], wd, s02);
                            s13 = __builtin_elementwise_fma(pb[d - 1], wd, s13);
                        }
                        const float sj[4] = {s02.x, s13.x, s02.y, s13.y};
                        const uint32_t gw = G[(k + 1) % 6];  // row t - 5
                        uint32_t m = 0;
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int mean = clampi((int)__builtin_rintf(sj[j]), 0, 255);
                            if (x + j < W && (int)byte_of(gw, j) - mean <= -2) m |= 1u << j;
                        }
                        // the 8 lanes of a half row (32 columns) OR their nibbles into one dword:
                        // xor 1, xor 2 within quads, then the mirrored half row
                        uint32_t v = m << (4 * (lane & 7));
                        v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
                        v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
                        v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, true);  // row_half_mirror
                        if (store_lane) out[(size_t)yo * wpr * 2 + (x >> 5)] = v;
                    }
                }
            }
        }
    }
}

}  // namespace

void font_bits_tiling(int h, int w, int *strips, int *segs, int *seg_rows) {
    *strips = (w + kStripW - 1) / kStripW;
    int sg = std::max(1, (h + kSegRows - 1) / kSegRows);
    const int rows = (h + sg - 1) / sg;
    sg = (h + rows - 1) / rows;
    *segs = sg;
    *seg_rows = rows;
}
int font_bits_strip_width() { return kStripW; }

hipError_t launch_font_bits(const uint8_t *bgr, const uint64_t *img_tab, int n, int h, int w, uint64_t *bits,
                            hipStream_t s) {
    if (n <= 0) return hipSuccess;
    int strips, segs, seg_rows;
    font_bits_tiling(h, w, &strips, &segs, &seg_rows);
    const long long waves = (long long)n * strips * segs;
    if (waves > 0x7fffffffll - kWavesPerBlock) return hipErrorInvalidValue;
    const int blocks = (int)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(k_font_bits, dim3(blocks), dim3(64 * kWavesPerBlock), 0, s, bgr, img_tab, h, w, strips, segs,
                       seg_rows, (int)waves, words_per_row(w), bits);
    return hipGetLastError();
}

}  // namespace llfe
