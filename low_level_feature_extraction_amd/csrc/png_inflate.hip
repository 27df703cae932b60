// PNG decode on the device (llfe_png_decode_device; DESIGN.md §3 "PNG decode on the device"):
// the staged deflate streams of a batch -> the inflated filtered rows (raw) -> the BGR batch.
//
// k_png_inflate: one wave per image, running the block decoder of png_inflate_core.h with a
// sink that keeps the 32 KiB window in an LDS ring.  The symbol decode is wave-uniform and
// sequential (one table lookup, then a broadcast); what is parallel is the copying: a match is
// copied by all lanes (lane i reads ring[pos - dist + i % dist], so a copy that overlaps itself
// needs no second pass), a stored block 256 bytes at a time, and the ring leaves for raw in
// whole 256-byte pieces, a dword per lane.  Match sources therefore never come from global
// memory the wave has just written.  The Adler-32 rides on those pieces (core: adler_dword):
// each lane sums what it stores, the wave adds up at the end and compares with the file's.
// Ring 32 KiB + two tables 5.2 KiB + lengths: 38 436 B of LDS per wave, four waves per CU.
//
// k_png_unfilter_bgr: one wave per image, 64 rows at a time as a skewed pipeline: lane j owns
// row base + j and at step t produces pixel t - j.  The pixel above is what lane j - 1
// produced one step earlier (a lane shift), the pixel above left what it produced two steps
// earlier (the previous step's shift, kept), the pixel to the left the lane's own last
// result: no memory traffic for the recurrence.  Lane 0 of a band behind the first reads the
// row above from the output the previous band wrote.  The filter type is a per-lane select.
// Alpha takes part in nothing that is kept, so its bytes are not even loaded.  Pixels are
// unfiltered straight in BGR order (the filters are per channel).
//
// Every index derives from descriptors the host validated (validate_png_descs); everything an
// image's wave writes lies in its own raw row and its own output image.
#include "llfe_internal.h"
#include "png_inflate_core.h"

namespace llfe {
namespace {

using namespace llfe_png;
constexpr uint32_t kRingMask = kWindow - 1;
constexpr uint32_t kPiece = 256;  // bytes the ring hands to raw at a time: one dword per lane

struct RingSink {
    uint8_t *ring;  // LDS, kWindow bytes
    uint8_t *raw;   // the image's row of raw_dev, 16-byte aligned
    uint32_t raw_n;
    uint32_t n;        // bytes produced
    uint32_t flushed;  // bytes stored to raw, a multiple of kPiece until finish()
    uint32_t pieces;
    int ln;
    uint64_t ad_a, ad_b;  // this lane's share of the Adler sums

    __device__ int lane() const { return ln; }
    __device__ int lanes() const { return 64; }
    __device__ void sync() { __syncthreads(); }
    __device__ uint32_t uniform(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ uint32_t pos() const { return n; }

    __device__ void flush() {
        if (n - flushed < kPiece) return;
        __syncthreads();  // the ring bytes are written
        while (n - flushed >= kPiece) {
            const uint32_t g = flushed + 4u * (uint32_t)ln;
            const uint32_t v = *reinterpret_cast<const uint32_t *>(ring + (g & kRingMask));
            *reinterpret_cast<uint32_t *>(raw + g) = v;
            adler_dword(ad_a, ad_b, v, g, raw_n);
            if ((++pieces & 255u) == 0) {
                ad_a %= kAdlerMod;
                ad_b %= kAdlerMod;
            }
            flushed += kPiece;
        }
    }
    __device__ void literal(uint8_t b) {
        if (ln == 0) ring[n & kRingMask] = b;
        n++;
        flush();
    }
    __device__ void match(uint32_t dist, uint32_t len) {
        __syncthreads();  // the source bytes are written
        const uint32_t from = n - dist;
        for (uint32_t i = (uint32_t)ln; i < len; i += 64) {
            const uint32_t k = dist >= len ? i : i % dist;  // (a copy that overlaps itself is periodic)
            ring[(n + i) & kRingMask] = ring[(from + k) & kRingMask];
        }
        n += len;
        flush();
    }
    __device__ void stored(const uint8_t *src, uint32_t len) {
        for (uint32_t o = 0; o < len; o += kPiece) {  // (never more unflushed bytes than a piece and a match)
            const uint32_t m = len - o < kPiece ? len - o : kPiece;
            for (uint32_t i = (uint32_t)ln; i < m; i += 64) ring[(n + i) & kRingMask] = src[o + i];
            n += m;
            flush();
        }
    }
    // the bytes behind the last whole piece
    __device__ void finish() {
        __syncthreads();
        for (uint32_t g = flushed + (uint32_t)ln; g < n; g += 64) {
            const uint32_t d = ring[g & kRingMask];
            raw[g] = (uint8_t)d;
            adler_byte(ad_a, ad_b, d, g, raw_n);
        }
        flushed = n;
    }
};

__device__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(64) void k_png_inflate(const uint8_t *__restrict__ staging, const llfe_png_desc *__restrict__ descs,
                                                    uint8_t *__restrict__ raw, long long raw_stride, int *__restrict__ status) {
    __shared__ __align__(16) uint8_t ring[kWindow];
    __shared__ Tables T;
    const int img = blockIdx.x;
    if (status[img] != 0) return;
    const llfe_png_desc d = descs[img];
    Reader r;
    rd_init(r, staging + d.record_offset, (uint32_t)d.deflate_bytes);
    RingSink s{ring, raw + (long long)img * raw_stride, (uint32_t)d.raw_bytes, 0, 0, 0, (int)threadIdx.x, 0, 0};
    int rc = inflate(r, T, s, s.raw_n);
    s.finish();
    if (rc == kOk) {
        // a = 1 + the sum of the bytes, b = n + the weighted sum (core: adler_dword)
        const uint32_t a = (wave_sum((uint32_t)(s.ad_a % kAdlerMod)) + 1u) % kAdlerMod;
        const uint32_t b = (wave_sum((uint32_t)(s.ad_b % kAdlerMod)) + s.raw_n % kAdlerMod) % kAdlerMod;
        if ((b << 16 | a) != d.adler) rc = kEAdler;
    }
    if (rc != kOk && threadIdx.x == 0) status[img] = LLFE_ERR_UNSUPPORTED;
}

// three bytes -> bits 0..23
__device__ __forceinline__ uint32_t ld_bgr(const uint8_t *p) { return (uint32_t)p[2] | (uint32_t)p[1] << 8 | (uint32_t)p[0] << 16; }

__global__ __launch_bounds__(64) void k_png_unfilter_bgr(const uint8_t *__restrict__ raw, long long raw_stride,
                                                         const llfe_png_desc *__restrict__ descs, int h, int w, uint8_t *out,
                                                         int *__restrict__ status) {
    const int img = blockIdx.x, lane = threadIdx.x;
    if (status[img] != 0) return;
    const llfe_png_desc d = descs[img];
    const long long stride = (long long)d.row_bytes + 1;
    const uint8_t *src = raw + (long long)img * raw_stride;
    uint8_t *o = out + (long long)img * h * w * 3;
    bool bad = false;
    for (int base = 0; base < h; base += 64) {
        const int y = base + lane;
        const bool active = y < h;
        int f = active ? src[y * stride] : 0;
        if (f > 4) {
            bad = true;
            f = 0;
        }
        const uint8_t *sp = src + (active ? y : 0) * stride + 1;
        uint8_t *op = o + (long long)(active ? y : 0) * w * 3;
        const uint8_t *upp = op - (long long)w * 3;  // (read by lane 0 of a later band only)
        uint32_t a = 0, b_prev = 0, mine = 0;
        for (int t = 0; t < w + 63; t++) {
            const int x = t - lane;
            uint32_t b = __shfl_up(mine, 1);  // pixel x of the row above: lane - 1's result of step t - 1
            const bool in = active && x >= 0 && x < w;
            if (lane == 0) {
                b = 0;
                if (base > 0 && in)  // the previous band's last row, past this CU's vector cache
                    b = (uint32_t)__hip_atomic_load(upp + 3 * x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
                        (uint32_t)__hip_atomic_load(upp + 3 * x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 8 |
                        (uint32_t)__hip_atomic_load(upp + 3 * x + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 16;
            }
            if (in) {
                const uint32_t c = x > 0 ? b_prev : 0;
                a = unfilter_px(f, ld_bgr(sp + (long long)x * d.bpp), a, b, c);
                uint8_t *q = op + 3 * (long long)x;  // (three byte stores: nothing past the row's last byte)
                q[0] = (uint8_t)a;
                q[1] = (uint8_t)(a >> 8);
                q[2] = (uint8_t)(a >> 16);
                mine = a;
                b_prev = b;
            }
        }
        __threadfence();  // this band's last row is in memory before the next band reads it
    }
    if (__any(bad) && lane == 0) status[img] = LLFE_ERR_UNSUPPORTED;
}

}  // namespace

hipError_t launch_png_decode(int stage, const uint8_t *staging, const llfe_png_desc *d_descs, int n, int h, int w,
                             uint8_t *raw, int64_t raw_stride, uint8_t *out, int *d_status, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (stage == 0)
        hipLaunchKernelGGL(k_png_inflate, dim3(n), dim3(64), 0, s, staging, d_descs, raw, (long long)raw_stride, d_status);
    else
        hipLaunchKernelGGL(k_png_unfilter_bgr, dim3(n), dim3(64), 0, s, raw, (long long)raw_stride, d_descs, h, w, out,
                           d_status);
    return hipGetLastError();
}

}  // namespace llfe
