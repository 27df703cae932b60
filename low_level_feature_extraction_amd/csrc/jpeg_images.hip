// JPEG reconstruction of a batch whose images each have their own size and sampling class
// (llfe_jpeg_reconstruct_images, and llfe_jpeg_reconstruct with every image of one size):
// quantised coefficients in slots (staged by llfe_jpeg_read_coefs_images or
// llfe_jpeg_read_coefs_batch, jpeg_decode.cpp) -> each image's packed H x W x 3 BGR result,
// bit for bit what the host decoder writes.
//
// One launch over a host-built work table of (image, tile) entries; images that were not
// staged have no entries.  A workgroup reconstructs one tile (jpeg_images.h JpegTiling) of
// one image end to end:
//   1. eight lanes per 8x8 block, 32 blocks per pass, a fixed number of passes per class:
//      the luma blocks of the tile, then the chroma blocks of the tile and of its halo, are
//      dequantised and inverse-transformed (jpeg_recon_core.h idct_block_row) and their u8
//      samples stored into planes in LDS.  A block outside the component's grid is skipped:
//      no load, no store.
//   2. four pixels of one row per lane: 4 luma bytes in one LDS load, the chroma
//      neighbourhood of two columns at coordinates clamped to the component's real
//      width - 1 / height - 1 (libjpeg's first / last column and row rules), so every sample
//      read lies in a block that pass 1 stored; h2v1 / h2v2 / replication, YCbCr -> BGR,
//      12 bytes out.
// No plane byte goes through HBM and there is no plane workspace.
//
// EXIF orientation (jpeg_orient.h) only changes where step 2 stores, so the kernel is a template
// on the orientation group and the host launches each group over its own part of the work table:
//   G = 0  orientation 1: the code above, unchanged.
//   G = 1  orientations 2, 3, 4: the result keeps its shape; a lane's row goes to the mirrored
//          row, its four pixels, reversed inside their 12 bytes, to the mirrored columns.
//   G = 2  orientations 5 .. 8: the result is w x h, so a row of the tile is a column of the
//          result.  The tile's pixels are staged in LDS in result order, one dword per pixel (in
//          the IDCT scratch of step 1, enlarged), and after a barrier step 3 writes every result
//          row of the tile as one contiguous run of th * 3 bytes.  Staging row lx (a result row)
//          starts at lx * (th + 3) + 2 * (lx >> 6) dwords: with the odd pitch the 16 lanes of a
//          tile row that write one staging column fall on 16 banks four apart, the two halves of
//          a 128-pixel row two banks apart and consecutive tile rows one bank apart, and step 3's
//          reads of four consecutive staging rows fall in four different bank classes mod 4.
//
// Every index derives from a record that the entry point validated on the host
// (llfe_decode.cpp): the descriptor against the image's own size and slot, the slot inside the
// coefficient buffer, the result inside the output and apart from every other image's.
#include "jpeg_images.h"
#include "jpeg_orient.h"
#include "jpeg_recon_core.h"
#include "llfe_internal.h"

namespace llfe {
namespace {

using namespace jpeg_core;

// the 12 bytes of pixels x0 .. x0 + 3 of a coded row of width w, already in reversed order in px
// (pixel x0 + 3 first), to the row `row` mirrored: the pixels that exist end at column w - 1 - x0
__device__ __forceinline__ void store_bgr4_mirrored(uint8_t *row, const uint3 px, int vec, int x0, int w) {
    const int npx = min(4, w - x0), skip = 12 - 3 * npx;
    uint8_t *o = row + (int64_t)(w - x0 - npx) * 3;
    if (vec && npx == 4) {
        unsigned *o4 = (unsigned *)o;
        o4[0] = px.x;
        o4[1] = px.y;
        o4[2] = px.z;
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++)
            if (k >= skip) o[k - skip] = (uint8_t)((k < 4 ? px.x : k < 8 ? px.y : px.z) >> (8 * (k & 3)));
    }
}

// G: the orientation group of every image of the launch (jpeg_orient_group)
template <int G>
__global__ __launch_bounds__(JT) void k_jpeg_images(const uint8_t *__restrict__ coefs,
                                                    const JpegImageRec *__restrict__ recs,
                                                    const JpegWork *__restrict__ work, uint8_t *__restrict__ out) {
    __shared__ int tile[G == 2 ? kJpegOrientStageTiles : kBlocksPerPass][8][9];
    __shared__ __align__(16) uint8_t yp[kJpegImgYBytes];
    __shared__ __align__(16) uint8_t cp[2][kJpegImgCBytes];
    const JpegWork wk = work[blockIdx.x];
    const JpegImageRec &R = recs[wk.image];
    const llfe_jpeg_desc &d = R.d;
    const int cls = d.sampling;
    JpegTiling T;
    if (!jpeg_tiling(cls, &T)) return;  // (whole workgroup; the host refused such a class)
    const int ty = wk.tile / R.tiles_x, tx = wk.tile - ty * R.tiles_x;
    const int x_org = tx * T.tw, y_org = ty * T.th;
    // the first luma block of the tile, and the first chroma block the tile keeps (halo included)
    const int ybx0 = x_org >> 3, yby0 = y_org >> 3;
    const int hsub = cls == LLFE_JPEG_422 || cls == LLFE_JPEG_420, vsub = cls == LLFE_JPEG_420;
    const int cbx0 = (x_org >> (3 + hsub)) - T.hx, cby0 = (y_org >> (3 + vsub)) - T.hy;
    const uint8_t *slot = coefs + R.slot_offset;

    {  // 1. the tile's blocks -> u8 planes in LDS
        const int g = threadIdx.x >> 3, j = threadIdx.x & 7;
        const int nY = T.tbw * T.tbh, nC = T.cbw * T.cbh;
        const int total = nY + (d.n_comp == 3 ? 2 * nC : 0);
        for (int b0 = 0; b0 < total; b0 += kBlocksPerPass) {
            int r = b0 + g, c = 0, bwl = T.tbw;
            bool act = r < total;
            if (r >= nY) {
                r -= nY;
                c = 1;
                if (r >= nC) {
                    r -= nC;
                    c = 2;
                }
                bwl = T.cbw;
            }
            c = act ? c : 0;
            const int ly = act ? r / bwl : 0, lx = act ? r - ly * bwl : 0;
            const int gx = (c ? cbx0 : ybx0) + lx, gy = (c ? cby0 : yby0) + ly;
            const int bw = d.comp[c].blocks_w;
            act = act && gx >= 0 && gy >= 0 && gx < bw && gy < d.comp[c].blocks_h;  // never a block outside the grid
            uint4 raw = make_uint4(0, 0, 0, 0), q = raw;
            if (act) {
                raw = *(const uint4 *)(slot + d.comp[c].coef_offset + ((int64_t)gy * bw + gx) * 128 + j * 16);
                q = *(const uint4 *)(slot + d.comp[c].quant_offset + j * 16);
            }
            const uint2 row = idct_block_row(tile[g], raw, q, j);
            if (act) {
                uint8_t *plane = c ? cp[c - 1] : yp;
                *(uint2 *)(plane + (ly * 8 + j) * (c ? T.cpitch : T.ypitch) + lx * 8) = row;
            }
        }
    }
    __syncthreads();

    // 2. upsampling and colour conversion from LDS
    const int h = R.h, w = R.w;
    const int lanes_shift = T.tw == 128 ? 5 : 4;  // lanes per tile row = tw / 4
    const int rows_per_pass = JT >> lanes_shift;
    const int rx = (threadIdx.x & ((1 << lanes_shift) - 1)) * 4;
    const int x0 = x_org + rx;
    if (G != 2 && x0 >= w) return;  // (no barrier below; G == 2: such a lane only skips step 2)
    uint8_t *o_img = out + R.out_offset;
    const int dw = d.comp[1].width, dh = d.comp[1].height;  // (read for 4:2:2 and 4:2:0 only)
    const int cx_org = cbx0 * 8, cy_org = cby0 * 8;         // the chroma sample at LDS (0, 0)
    const int ori = G == 0 ? 1 : R.orient;
    // G == 2: the tile's real pixels, the staging pitch in dwords, and the result column at which
    // the runs of the tile start (its first or its last row, whichever the orientation puts first)
    const int vw = min(T.tw, w - x_org), vh = min(T.th, h - y_org);
    const int spitch = T.th + 3;
    unsigned *stage = (unsigned *)tile;  // (step 1 is done with it)
    int col0 = 0;
    if constexpr (G == 2) {
        int ya, xa, yb, xb;
        jpeg_orient_map(ori, h, w, y_org, x_org, &ya, &xa);
        jpeg_orient_map(ori, h, w, y_org + vh - 1, x_org, &yb, &xb);
        col0 = min(xa, xb);
    }
    for (int r0 = (G == 2 && x0 >= w) ? T.th : 0; r0 < T.th; r0 += rows_per_pass) {
        const int ry = r0 + (threadIdx.x >> lanes_shift);
        const int y = y_org + ry;
        if (y >= h) break;
        const unsigned y4 = *(const unsigned *)(yp + ry * T.ypitch + rx);
        int4 cb = make_int4(128, 128, 128, 128), cr = cb;  // (grey)
        if (cls == LLFE_JPEG_444) {
            cb = bytes4(*(const unsigned *)(cp[0] + ry * T.cpitch + rx));
            cr = bytes4(*(const unsigned *)(cp[1] + ry * T.cpitch + rx));
        } else if (cls != LLFE_JPEG_GRAY) {
            // global chroma coordinates, clamped to the component's real samples, then made local
            const bool v2 = cls == LLFE_JPEG_420;
            const int cy = v2 ? y >> 1 : y;
            const int fy = !v2 ? cy : (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);
            const int g0 = x0 >> 1;
            const int c0 = g0 - cx_org, c1 = min(g0 + 1, dw - 1) - cx_org, cm = max(g0 - 1, 0) - cx_org,
                      c2 = min(g0 + 2, dw - 1) - cx_org;
            const int no = (cy - cy_org) * T.cpitch, fo = (fy - cy_org) * T.cpitch;
            cb = upsample4(cp[0] + no, cp[0] + fo, cm, c0, c1, c2, v2, dw <= 2);
            cr = upsample4(cp[1] + no, cp[1] + fo, cm, c0, c1, c2, v2, dw <= 2);
        }
        if constexpr (G == 0) {
            store_bgr4(o_img + ((int64_t)y * w + x0) * 3, ycc_to_bgr4(y4, cb, cr), R.vec, x0, w);
        } else if constexpr (G == 1) {
            int yr, xr;
            jpeg_orient_map(ori, h, w, y, x0, &yr, &xr);
            uint8_t *row = o_img + (int64_t)yr * w * 3;
            if (jpeg_orient_mirror_x(ori))
                store_bgr4_mirrored(row, ycc_to_bgr4(__builtin_bswap32(y4), make_int4(cb.w, cb.z, cb.y, cb.x),
                                                     make_int4(cr.w, cr.z, cr.y, cr.x)), R.vec, x0, w);
            else
                store_bgr4(row + (int64_t)x0 * 3, ycc_to_bgr4(y4, cb, cr), R.vec, x0, w);
        } else {
            // a dword per pixel into the staging row of its column, at its place in that row's run
            const uint3 px = ycc_to_bgr4(y4, cb, cr);
            int yr, xr;
            jpeg_orient_map(ori, h, w, y, x0, &yr, &xr);
            unsigned *sp = stage + rx * spitch + 2 * (rx >> 6) + (xr - col0);
            sp[0] = px.x & 0xffffffu;
            sp[spitch] = px.x >> 24 | (px.y & 0xffffu) << 8;
            sp[2 * spitch] = px.y >> 16 | (px.z & 0xffu) << 16;
            sp[3 * spitch] = px.z >> 8;
        }
    }
    if constexpr (G == 2) {
        __syncthreads();
        // 3. every result row of the tile: a run of vh pixels, four per lane, from the staging row
        // of the coded column it comes from
        const int run_shift = T.th == 64 ? 4 : 3;  // lanes per run = th / 4
        const int q4 = (threadIdx.x & ((1 << run_shift) - 1)) * 4;
        if (q4 >= vh) return;
        for (int l0 = 0; l0 < T.tw; l0 += JT >> run_shift) {
            const int lx = l0 + (threadIdx.x >> run_shift);
            if (lx >= vw) break;
            const unsigned *sp = stage + lx * spitch + 2 * (lx >> 6) + q4;
            const unsigned p0 = sp[0], p1 = sp[1], p2 = sp[2], p3 = sp[3];  // (past vh: staging room, not stored)
            int yr, xr;
            jpeg_orient_map(ori, h, w, y_org, x_org + lx, &yr, &xr);
            store_bgr4(o_img + ((int64_t)yr * h + col0 + q4) * 3,
                       make_uint3(p0 | p1 << 24, p1 >> 8 | p2 << 16, p2 >> 16 | p3 << 8), R.vec, q4, vh);
        }
    }
}

}  // namespace

hipError_t launch_jpeg_images(const uint8_t *coefs, const JpegImageRec *d_recs, const JpegWork *d_work, int n_work,
                              uint8_t *out, int group, hipStream_t s) {
    if (n_work <= 0) return hipSuccess;
    const dim3 grid((unsigned)n_work), block(JT);
    switch (group) {
    case 0: hipLaunchKernelGGL(k_jpeg_images<0>, grid, block, 0, s, coefs, d_recs, d_work, out); break;
    case 1: hipLaunchKernelGGL(k_jpeg_images<1>, grid, block, 0, s, coefs, d_recs, d_work, out); break;
    case 2: hipLaunchKernelGGL(k_jpeg_images<2>, grid, block, 0, s, coefs, d_recs, d_work, out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace llfe
