// The host check of llfe_jpeg_desc records, in front of every kernel that indexes a coefficient
// slot through them: llfe_jpeg_reconstruct and llfe_jpeg_reconstruct_images (jpeg_images.hip),
// llfe_jpeg_entropy_decode (jpeg_huff.hip) and the latter's host twin (jpeg_decode.cpp, which is
// also built on its own without the device code).  Plain C++, no HIP types.
#ifndef LLFE_JPEG_DESC_CHECK_H
#define LLFE_JPEG_DESC_CHECK_H
#include <algorithm>
#include <cstdint>

#include "llfe.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LLFE_DESC_HD __host__ __device__ inline
#else
#define LLFE_DESC_HD inline
#endif

namespace llfe {

// one staged descriptor (n_comp != 0) against (h, w) and the bytes of its slot: false for any
// offset or extent outside the slot, a block grid that does not cover the image or an unknown
// sampling class; on success the largest block count of a component
inline bool check_jpeg_desc(const llfe_jpeg_desc &d, int h, int w, int64_t slot_bytes, int64_t *max_blocks) {
    auto div_up = [](int a, int b) { return (a + b - 1) / b; };
    const int cls = d.sampling;
    int64_t mb = 0;
    if (!((d.n_comp == 1 && cls == LLFE_JPEG_GRAY) ||
          (d.n_comp == 3 && (cls == LLFE_JPEG_444 || cls == LLFE_JPEG_422 || cls == LLFE_JPEG_420))))
        return false;
    for (int c = 0; c < d.n_comp; c++) {
        const auto &k = d.comp[c];
        const int hs = c && (cls == LLFE_JPEG_422 || cls == LLFE_JPEG_420) ? 2 : 1;
        const int vs = c && cls == LLFE_JPEG_420 ? 2 : 1;
        // the component's real samples and a block grid that covers them
        if (k.width != div_up(w, hs) || k.height != div_up(h, vs)) return false;
        if (k.blocks_w < div_up(k.width, 8) || k.blocks_h < div_up(k.height, 8) || k.blocks_w > 8192 ||
            k.blocks_h > 8192)
            return false;
        const int64_t bytes = (int64_t)k.blocks_w * k.blocks_h * 128;
        if (k.coef_offset < 0 || (k.coef_offset & 15) || k.coef_offset > slot_bytes ||
            bytes > slot_bytes - k.coef_offset)
            return false;
        if (k.quant_offset < 0 || (k.quant_offset & 15) || k.quant_offset > slot_bytes ||
            128 > slot_bytes - k.quant_offset)
            return false;
        mb = std::max<int64_t>(mb, (int64_t)k.blocks_w * k.blocks_h);
    }
    if (d.n_comp == 3 && (d.comp[1].blocks_w != d.comp[2].blocks_w || d.comp[1].blocks_h != d.comp[2].blocks_h))
        return false;
    *max_blocks = mb;
    return true;
}

// n descriptors against (h, w) and the slot stride: false when check_jpeg_desc refuses one of
// the staged ones
inline bool check_jpeg_descs(const llfe_jpeg_desc *descs, int n, int h, int w, int64_t slot_stride) {
    for (int i = 0; i < n; i++) {
        int64_t blocks = 0;
        if (descs[i].n_comp != 0 && !check_jpeg_desc(descs[i], h, w, slot_stride, &blocks)) return false;
    }
    return true;
}

}  // namespace llfe
#endif
