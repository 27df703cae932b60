// JPEG reconstruction of a batch whose images each have their own size and sampling class
// (llfe_jpeg_reconstruct_images): quantised coefficients in tight slots (staged by
// llfe_jpeg_read_coefs_images, jpeg_decode.cpp) -> each image's packed H x W x 3 BGR result,
// bit for bit what jpeg_recon.hip and the host decoder write.
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
// Every index derives from a record that llfe_jpeg_reconstruct_images validated on the host:
// the descriptor against the image's own size and slot, the slot inside the coefficient
// buffer, the result inside the output and apart from every other image's.
#include "jpeg_images.h"
#include "jpeg_recon_core.h"
#include "llfe_internal.h"

namespace llfe {
namespace {

using namespace jpeg_core;

__global__ __launch_bounds__(JT) void k_jpeg_images(const uint8_t *__restrict__ coefs,
                                                    const JpegImageRec *__restrict__ recs,
                                                    const JpegWork *__restrict__ work, uint8_t *__restrict__ out) {
    __shared__ int tile[kBlocksPerPass][8][9];
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
    if (x0 >= w) return;  // (no barrier below)
    uint8_t *o_img = out + R.out_offset;
    const int dw = d.comp[1].width, dh = d.comp[1].height;  // (read for 4:2:2 and 4:2:0 only)
    const int cx_org = cbx0 * 8, cy_org = cby0 * 8;         // the chroma sample at LDS (0, 0)
    for (int r0 = 0; r0 < T.th; r0 += rows_per_pass) {
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
        store_bgr4(o_img + ((int64_t)y * w + x0) * 3, ycc_to_bgr4(y4, cb, cr), R.vec, x0, w);
    }
}

}  // namespace

hipError_t launch_jpeg_images(const uint8_t *coefs, const JpegImageRec *d_recs, const JpegWork *d_work, int n_work,
                              uint8_t *out, hipStream_t s) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_jpeg_images, dim3((unsigned)n_work), dim3(JT), 0, s, coefs, d_recs, d_work, out);
    return hipGetLastError();
}

}  // namespace llfe
