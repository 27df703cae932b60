// FontDetector.detect_font after preprocess_image (app/services/analyze/font_detector.py
// :39-67 detect_text_regions, :109-155 detect_font) on the GPU.  The binary (stencil.hip's
// font path, or the caller's) is packed into bit rows, the boxes-only mode of the contour
// pass (contours_gpu.hip) gives every external contour's bounding box in OpenCV's order,
// and the kernels here turn them into one small record per image:
//
//   k_font_pack      u8 binary -> u64 bit rows, one ballot per word
//   k_font_select    one workgroup per image walks its contours in cv2 order (newest start
//                    first): the filter 0.1 < w / float(h) < 15 and h > 8, the region
//                    count, and max(regions, key = w * h) with Python's "first maximum wins"
//   k_font_regions   (only when the list is wanted) the kept boxes, compacted in order
//   k_font_gray_sum  sum of cvtColor(BGR2GRAY) over the winning rectangle
//
// Everything is integer arithmetic, so no result depends on the order of the reductions.
// The aspect filter is the integer test 10 w > h and w < 15 h: w / float(h) is a
// correctly rounded double, and for w <= 4096, h <= 65535 a ratio that differs from 0.1
// (or 15) differs by at least 1 / (10 h), far above a double ulp, so the rounded quotient
// compares as the exact one does.
#include <algorithm>

#include "../../include/llfe.h"
#include "llfe_internal.h"

namespace llfe {
namespace {

constexpr int NT = 256, NW = NT / 64;
// max of (w * h) << 30 | (2^30 - 1 - k): the largest area, earliest list index k on ties
// (w * h <= 4096 * 65535 < 2^28; an image has fewer than 2^31 / 4 external contours)
constexpr uint64_t kIdxMask = (1ull << 30) - 1;

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the bounding box of contour k (cv2 list order) of an image whose refs start at base
__device__ __forceinline__ int4 box_of(const CtComp *comps, const int2 *refs, int base, int nref, int k) {
    const CtComp c = comps[refs[base + nref - 1 - k].x];
    return make_int4(c.x0, c.y0, c.x1 - c.x0 + 1, c.y1 - c.y0 + 1);
}
__device__ __forceinline__ bool is_text_region(const int4 b) {
    return 10 * b.z > b.w && b.z < 15 * b.w && b.w > 8;
}

// one wave per 64-pixel word: lanes read consecutive bytes, the ballot is the word
__global__ __launch_bounds__(NT) void k_font_pack(const uint8_t *__restrict__ mask, int64_t rows, int w, int wpr,
                                                  uint64_t *__restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int64_t words = rows * wpr;
    for (int64_t i = (int64_t)blockIdx.x * NW + (threadIdx.x >> 6); i < words; i += (int64_t)gridDim.x * NW) {
        const int64_t r = i / wpr;
        const int x = (int)(i - r * wpr) * 64 + lane;
        const bool on = x < w && mask[r * w + x] != 0;
        const uint64_t b = __ballot(on);
        if (lane == 0) bits[i] = b;
    }
}

__global__ __launch_bounds__(NT) void k_font_select(const CtComp *__restrict__ comps, const int2 *__restrict__ refs,
                                                    const int *__restrict__ img_info,
                                                    llfe_font_result *__restrict__ rec) {
    __shared__ uint64_t s_best[NW];
    __shared__ int s_cnt[NW];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int base = img_info[img * kCtInfo + 1], nref = img_info[img * kCtInfo + 2];
    uint64_t best = 0;
    int cnt = 0;
    for (int k = tid; k < nref; k += NT) {
        const int4 b = box_of(comps, refs, base, nref, k);
        if (!is_text_region(b)) continue;
        cnt++;
        const uint64_t key = ((uint64_t)(b.z * b.w) << 30) | (kIdxMask - (uint64_t)k);
        best = key > best ? key : best;
    }
    best = wave_max_u64(best);
    cnt = wave_sum_i32(cnt);
    if ((tid & 63) == 0) {
        s_best[tid >> 6] = best;
        s_cnt[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < NW; i++) {
            best = s_best[i] > best ? s_best[i] : best;
            cnt += s_cnt[i];
        }
        llfe_font_result r;
        r.n_contours = nref;
        r.n_regions = cnt;
        r.x = r.y = r.width = r.height = 0;
        r.region_offset = 0;
        r.gray_sum = 0;
        if (cnt > 0) {
            const int4 b = box_of(comps, refs, base, nref, (int)(kIdxMask - (best & kIdxMask)));
            r.x = b.x;
            r.y = b.y;
            r.width = b.z;
            r.height = b.w;
        }
        rec[img] = r;
    }
}

// the kept boxes of image blockIdx.x at regions[sum of the earlier images' counts ...]
__global__ __launch_bounds__(NT) void k_font_regions(const CtComp *__restrict__ comps, const int2 *__restrict__ refs,
                                                     const int *__restrict__ img_info,
                                                     const llfe_font_result *__restrict__ rec,
                                                     int4 *__restrict__ regions, int64_t cap) {
    __shared__ unsigned long long s_off[NW];
    __shared__ int s_cnt[NW];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long off = 0;
    for (int i = tid; i < img; i += NT) off += (unsigned long long)rec[i].n_regions;
    off = wave_sum_u64(off);
    if (lane == 0) s_off[wv] = off;
    __syncthreads();
    int64_t pos = 0;
    for (int i = 0; i < NW; i++) pos += (int64_t)s_off[i];
    const int base = img_info[img * kCtInfo + 1], nref = img_info[img * kCtInfo + 2];
    for (int c0 = 0; c0 < nref; c0 += NT) {
        const int k = c0 + tid;
        int4 b = make_int4(0, 0, 0, 0);
        bool keep = false;
        if (k < nref) {
            b = box_of(comps, refs, base, nref, k);
            keep = is_text_region(b);
        }
        const uint64_t bal = __ballot(keep);
        __syncthreads();  // s_cnt of the previous chunk has been read
        if (lane == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
        for (int i = 0; i < NW; i++) {
            if (i < wv) before += s_cnt[i];
            total += s_cnt[i];
        }
        if (keep && pos + before < cap) regions[pos + before] = b;
        pos += total;
    }
}

// grid (G, n): the rows of image blockIdx.y's winning rectangle go round the waves of
// its G workgroups; exact u64 sum, one atomic per workgroup
// (img_tab, may be null: image i at img_tab[i] instead of bgr + i * H * W * 3)
__global__ __launch_bounds__(NT) void k_font_gray_sum(const uint8_t *__restrict__ bgr,
                                                      const uint64_t *__restrict__ img_tab, int H, int W,
                                                      llfe_font_result *rec) {
    __shared__ unsigned long long s_sum[NW];
    const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    struct {
        int n_regions, x, y, width, height;
    } r = {rec[img].n_regions, rec[img].x, rec[img].y, rec[img].width, rec[img].height};  // (not gray_sum: others add)
    if (r.n_regions <= 0|| r.width <= 0 || r.height <= 0) return;
    if (r.x < 0 || r.y < 0 || r.x + r.width > W || r.y + r.height > H) return;  // (never: boxes lie in the image)
    const uint8_t *im = img_tab ? (const uint8_t *)img_tab[img] : bgr + (size_t)img * H * W * 3;
    unsigned long long sum = 0;
    for (int row = blockIdx.x * NW + wv; row < r.height; row += gridDim.x * NW) {
        const uint8_t *p = im + ((size_t)(r.y + row) * W + r.x) * 3;
        uint32_t s = 0;  // a row of <= 4096 pixels: < 2^20
        for (int x = lane; x < r.width; x += 64) {
            const uint32_t b = p[3 * x], g = p[3 * x + 1], rr = p[3 * x + 2];
            s += (1868u * b + 9617u * g + 4899u * rr + 8192u) >> 14;
        }
        sum += s;
    }
    sum = wave_sum_u64(sum);
    if (lane == 0) s_sum[wv] = sum;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < NW; i++) sum += s_sum[i];
        if (sum) atomicAdd((unsigned long long *)&rec[img].gray_sum, sum);
    }
}

}  // namespace

hipError_t launch_font_pack(const uint8_t *mask, int n, int h, int w, uint64_t *bits, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int wpr = words_per_row(w);
    const int64_t rows = (int64_t)n * h, words = rows * wpr;
    const unsigned grid = (unsigned)std::min<int64_t>((words + NW - 1) / NW, 1 << 16);
    hipLaunchKernelGGL(k_font_pack, dim3(grid), dim3(NT), 0, s, mask, rows, w, wpr, bits);
    return hipGetLastError();
}

hipError_t launch_font_select(const CtComp *comps, const int2 *refs, const int *img_info, int n,
                              llfe_font_result *rec, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_font_select, dim3(n), dim3(NT), 0, s, comps, refs, img_info, rec);
    return hipGetLastError();
}

hipError_t launch_font_regions(const CtComp *comps, const int2 *refs, const int *img_info, int n,
                               const llfe_font_result *rec, int4 *regions, int64_t cap, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_font_regions, dim3(n), dim3(NT), 0, s, comps, refs, img_info, rec, regions, cap);
    return hipGetLastError();
}

hipError_t launch_font_gray_sum(const uint8_t *bgr, int n, int h, int w, llfe_font_result *rec, hipStream_t s,
                                const uint64_t *img_tab) {
    if (n <= 0) return hipSuccess;
    const int g = std::max(1, std::min(32, (h + NW - 1) / NW));
    hipLaunchKernelGGL(k_font_gray_sum, dim3(g, n), dim3(NT), 0, s, bgr, img_tab, h, w, rec);
    return hipGetLastError();
}

}  // namespace llfe
