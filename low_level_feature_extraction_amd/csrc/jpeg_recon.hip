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
#include "jpeg_recon_core.h"
#include "llfe_internal.h"

namespace llfe {
namespace {

using namespace jpeg_core;  // jpeg_recon_core.h: the arithmetic, shared with jpeg_images.hip
constexpr int kBlocksPerWg = kBlocksPerPass;

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
    uint4 raw = make_uint4(0, 0, 0, 0), q = raw;
    if (act) {
        raw = *(const uint4 *)(slot + d.comp[c].coef_offset + (int64_t)blk * 128 + j * 16);
        q = *(const uint4 *)(slot + d.comp[c].quant_offset + j * 16);
    }
    const uint2 row = idct_block_row(tile[g], raw, q, j);
    if (!act) return;
    const int by = blk / bw, bx = blk - by * bw;
    uint8_t *plane = planes + (int64_t)img * plane_stride + plane_offset(d, c);
    *(uint2 *)(plane + ((int64_t)by * 8 + j) * ((int64_t)bw * 8) + bx * 8) = row;
}

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
    int4 cb = make_int4(128, 128, 128, 128), cr = cb;  // (grey)
    const int cls = d.sampling;
    if (cls != LLFE_JPEG_GRAY) {
        const int pitch = d.comp[1].blocks_w * 8;  // (validated: both chroma components alike)
        const uint8_t *p1 = p0 + plane_offset(d, 1), *p2 = p0 + plane_offset(d, 2);
        if (cls == LLFE_JPEG_444) {
            cb = bytes4(*(const unsigned *)(p1 + (int64_t)y * pitch + x0));
            cr = bytes4(*(const unsigned *)(p2 + (int64_t)y * pitch + x0));
        } else {
            // the chroma neighbourhood of two columns, clamped at the component's real edges
            const int dw = d.comp[1].width, dh = d.comp[1].height;
            const bool v2 = cls == LLFE_JPEG_420;
            const int cy = v2 ? y >> 1 : y;
            const int fy = !v2 ? cy : (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);
            const int c0 = x0 >> 1, c1 = min(c0 + 1, dw - 1), cm = max(c0 - 1, 0), c2 = min(c0 + 2, dw - 1);
            cb = upsample4(p1 + (int64_t)cy * pitch, p1 + (int64_t)fy * pitch, cm, c0, c1, c2, v2, dw <= 2);
            cr = upsample4(p2 + (int64_t)cy * pitch, p2 + (int64_t)fy * pitch, cm, c0, c1, c2, v2, dw <= 2);
        }
    }
    store_bgr4(out + ((int64_t)img * h * w + (int64_t)y * w + x0) * 3, ycc_to_bgr4(y4, cb, cr), vec, x0, w);
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
