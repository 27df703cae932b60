// The entropy half of a baseline JPEG decode on the device: the scan's bytes (staged by
// llfe_jpeg_parse_batch, jpeg_decode.cpp) -> exactly the coefficient slots that
// llfe_jpeg_read_coefs_batch writes on the host, for llfe_jpeg_reconstruct (jpeg_recon.hip).
// The decoding itself -- bit reader, tables, one subsequence -- is jpeg_huff_core.h, shared
// with the host twin llfe_jpeg_entropy_reference.
//
// Huffman data has no entry points, so the scan is cut into subsequences of kSub bytes, one
// lane each, and the lanes find their entry states by iteration:
//   k_huff_init    zero the coefficient areas, copy the quantisation tables into the slots
//   k_huff_sync    pass 0: every lane decodes from its boundary with a guessed state (block 0
//                  of the MCU, DC next), lane 0 from the true one, and records its exit state
//                  and the blocks it completed.  Then rounds inside the workgroup (256 lanes,
//                  exit states exchanged through LDS, a barrier per round): a lane whose
//                  predecessor's exit state differs from its entry state decodes again from
//                  it.  A workgroup whose first lane holds the true state is final after at
//                  most 255 rounds, so after pass p workgroup p is.  Across workgroups the
//                  last exit state travels through a double-buffered boundary array, read by
//                  the next launch: workgroups of one launch never read each other's results.
//                  The number of launches is the largest workgroup count of an image, fixed
//                  on the host from the scan lengths; a workgroup with nothing to redo leaves
//                  after one round.  Images of flat colour never synchronise by themselves
//                  (at 4:2:0 the four luma blocks of an MCU are bit-identical, a lane stays
//                  one block out of phase for ever): the true state is carried through them
//                  lane by lane, which these rounds do.
//   k_huff_verify  one workgroup per image: the image is good only if every lane's entry
//                  state is its predecessor's exit state, lane 0 started from the true state,
//                  no lane met an anomaly, the last lane ended on the scan's last bit (or its
//                  1-padding) at an MCU boundary and the blocks add up to the frame's.  Also
//                  the exclusive scan of the block counts: each lane's first block.
//   k_huff_write   decodes again from the verified states: block index -> (component, row,
//                  column) through the MCU geometry, padding blocks of edge MCUs dropped,
//                  coefficients stored in natural order, DC differences (padding blocks
//                  included) to a side array in scan order.
//   k_huff_dc      one workgroup per image: per-component prefix sums over the DC differences
//                  of all blocks in scan order, scattered to the real blocks.
// Restart intervals.  Every kernel behind k_huff_init exists twice, <RST = false> for the images
// whose record has restart_interval 0 and <true> for the others; each instance skips the other's
// images, and the host launches an instance only when the batch has images for it, so a batch
// without restart intervals runs the launches and the code it always ran.  With RST the lanes
// cross markers (jpeg_huff_core.h) and keep, next to the block count, the Marks of their last
// decode; k_huff_verify scans the marker counts along with the block counts and accepts an
// image only if no lane's Marks are bad, the first marker of every lane is the one its ordinal k
// asks for (FF D0 + (k & 7), behind exactly (k + 1) * Ri * blocks_in_mcu blocks) and the markers
// are (MCUs - 1) / Ri in all; the later markers of a lane are checked against its first one by
// the decode itself.  k_huff_dc restarts its sums at every interval (a segmented scan).
// Everything an image's lanes write lies in its own slot and its own rows of the workspace.
// Every index derives from records and descriptors the host validated (validate_scans,
// validate_jpeg_descs); every loop has a bound that follows from the scan length.
#include "jpeg_huff_core.h"
#include "llfe_internal.h"

namespace llfe {
namespace {

using namespace llfe_huff;

constexpr int HT = 256;  // lanes (subsequences) per workgroup

__constant__ uint8_t c_nat[64] = {LLFE_JPEG_NATURAL_ORDER};

struct Ws {
    State *in, *out;  // n x max_sub
    int *cnt, *first;  // n x max_sub
    State *bnd;        // 2 x n x max_wg: the last exit state of each workgroup, double-buffered
    int16_t *dcd;      // n x max_blocks
    Marks *marks;      // n x max_sub (RST)
    int max_sub, max_wg, max_blocks;
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

Ws carve(uint8_t *base, int n, int max_sub, int max_blocks, size_t *bytes) {
    Ws w;
    w.max_sub = max_sub;
    w.max_wg = (max_sub + HT - 1) / HT;
    w.max_blocks = max_blocks;
    size_t o = 0;
    const size_t lanes = (size_t)n * (size_t)max_sub;
    w.in = (State *)(base + o), o += up16(lanes * sizeof(State));
    w.out = (State *)(base + o), o += up16(lanes * sizeof(State));
    w.cnt = (int *)(base + o), o += up16(lanes * sizeof(int));
    w.first = (int *)(base + o), o += up16(lanes * sizeof(int));
    w.bnd = (State *)(base + o), o += up16(2 * (size_t)n * (size_t)w.max_wg * sizeof(State));
    w.dcd = (int16_t *)(base + o), o += up16((size_t)n * (size_t)max_blocks * sizeof(int16_t));
    w.marks = (Marks *)(base + o), o += up16(lanes * sizeof(Marks));
    *bytes = o;
    return w;
}

// what every lane of an image indexes at run time, in LDS: the decode tables, the zigzag
// table, the scan record and the descriptor
struct Shared {
    Tab tabs[4];
    llfe_jpeg_scan sc;
    llfe_jpeg_desc d;
    uint8_t nat[64];
};

template <class T>
__device__ __forceinline__ void copy_words(T *dst, const void *src) {
    static_assert(sizeof(T) % 4 == 0, "whole dwords");
    for (int k = threadIdx.x; k < (int)(sizeof(T) / 4); k += HT) ((uint32_t *)dst)[k] = ((const uint32_t *)src)[k];
}

__device__ __forceinline__ void load_shared(Shared &S, const uint8_t *staging, const llfe_jpeg_scan *scan,
                                            const llfe_jpeg_desc *desc) {  // (whole workgroup)
    copy_words(&S.tabs, staging + scan->record_offset + scan->table_offset);
    copy_words(&S.sc, scan);
    copy_words(&S.d, desc);
    if (threadIdx.x < 64) S.nat[threadIdx.x] = c_nat[threadIdx.x];
    __syncthreads();
}

__global__ __launch_bounds__(HT) void k_huff_init(const uint8_t *__restrict__ staging,
                                                  const llfe_jpeg_scan *__restrict__ scans,
                                                  const llfe_jpeg_desc *__restrict__ descs, uint8_t *__restrict__ slots,
                                                  int64_t slot_stride) {
    const int img = blockIdx.y;
    const llfe_jpeg_scan &sc = scans[img];
    if (sc.blocks_in_mcu == 0) return;
    const llfe_jpeg_desc &d = descs[img];
    uint8_t *slot = slots + (int64_t)img * slot_stride;
    const uint8_t *rec = staging + sc.record_offset;
    if (blockIdx.x == 0 && (int)threadIdx.x < d.n_comp * 8) {
        const int c = threadIdx.x >> 3, j = threadIdx.x & 7;
        *(uint4 *)(slot + d.comp[c].quant_offset + j * 16) = *(const uint4 *)(rec + sc.quant_offset + c * 128 + j * 16);
    }
    for (int c = 0; c < d.n_comp; c++) {
        const int64_t vecs = (int64_t)d.comp[c].blocks_w * d.comp[c].blocks_h * 8;  // 16-byte stores
        uint4 *dst = (uint4 *)(slot + d.comp[c].coef_offset);
        for (int64_t k = (int64_t)blockIdx.x * HT + threadIdx.x; k < vecs; k += (int64_t)gridDim.x * HT)
            dst[k] = make_uint4(0, 0, 0, 0);
    }
}

template <bool RST>
__global__ __launch_bounds__(HT) void k_huff_sync(const uint8_t *__restrict__ staging,
                                                  const llfe_jpeg_scan *__restrict__ scans,
                                                  const llfe_jpeg_desc *__restrict__ descs, const int *__restrict__ status,
                                                  Ws w, int n, int pass) {
    __shared__ Shared S;
    __shared__ State lds_out[HT];
    const int img = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
    if (status[img] != 0 || (scans[img].restart_interval != 0) != RST) return;  // (whole workgroup)
    const int len = scans[img].scan_bytes, nsub = subsequences(len);
    if (g * HT >= nsub) return;  // (whole workgroup)
    load_shared(S, staging, &scans[img], &descs[img]);
    const llfe_jpeg_scan &sc = S.sc;
    const Tab *tabs = S.tabs;
    const uint8_t *nat = S.nat;
    const uint8_t *scan = staging + sc.record_offset + sc.scan_offset;
    const int i = g * HT + t;
    const bool act = i < nsub;
    const int64_t lane = (int64_t)img * w.max_sub + i;
    const int end = min(len, (i + 1) * kSub);
    const State start{0, 0}, none{kNone, 0};
    const Geometry geo{&sc, &S.d, nullptr};
    State in = none, out = none;
    int cnt = 0;
    Marks mk{0, 0, 0, 0};
    if (act) {
        if (pass == 0) {
            in = i ? State{sub_start<RST>(scan, len, i), 0} : start;
            out = decode_sub<false, RST>(scan, len, tabs, sc, in, end, &cnt, nat, geo, nullptr, 0, 0, &mk);
        } else {
            in = w.in[lane];
            out = w.out[lane];
            cnt = w.cnt[lane];
            if (RST) mk = w.marks[lane];
        }
    }
    // the exit state in front of this workgroup: what its predecessor left in the last launch
    State before = g == 0 ? start : none;
    if (g > 0 && pass > 0) before = w.bnd[((int64_t)(pass & 1) * n + img) * w.max_wg + g - 1];
    for (int r = 0; r < HT; r++) {
        lds_out[t] = out;
        __syncthreads();
        const State prev = t == 0 ? before : lds_out[t - 1];
        const bool redo = act && prev.pos != kNone && !same(prev, in);
        if (redo) {
            in = prev;
            out = decode_sub<false, RST>(scan, len, tabs, sc, in, end, &cnt, nat, geo, nullptr, 0, 0, &mk);
        }
        if (!__syncthreads_or(redo)) break;
    }
    if (act) {
        w.in[lane] = in;
        w.out[lane] = out;
        w.cnt[lane] = cnt;
        if (RST) w.marks[lane] = mk;
        if (t == HT - 1 || i == nsub - 1) w.bnd[((int64_t)((pass + 1) & 1) * n + img) * w.max_wg + g] = out;
    }
}

template <bool RST>
__global__ __launch_bounds__(HT) void k_huff_verify(const llfe_jpeg_scan *__restrict__ scans, int *__restrict__ status,
                                                    Ws w) {
    __shared__ int s_scan[HT];
    __shared__ int s_mark[RST ? HT : 1];
    const int img = blockIdx.x, t = threadIdx.x;
    if (status[img] != 0 || (scans[img].restart_interval != 0) != RST) return;  // (whole workgroup)
    const llfe_jpeg_scan &sc = scans[img];
    const int len = sc.scan_bytes, nsub = subsequences(len);
    const int total = sc.mcus_w * sc.mcus_h * sc.blocks_in_mcu;
    const int64_t row = (int64_t)img * w.max_sub;
    int bad = 0, carry = 0, mcarry = 0;  // mcarry: the markers in front of this round's lanes
    for (int base = 0; base < nsub; base += HT) {
        const int i = base + t;
        int c = 0;
        Marks mk{0, 0, 0, 0};
        if (i < nsub) {
            const State o = w.out[row + i], e = w.in[row + i];
            const State prev = i ? w.out[row + i - 1] : State{0, 0};
            if (o.pos == kNone || !same(e, prev)) bad = 1;
            c = w.cnt[row + i];
            if (RST) mk = w.marks[row + i];
        }
        s_scan[t] = c;
        if (RST) s_mark[t] = mk.n;
        __syncthreads();
        for (int off = 1; off < HT; off <<= 1) {
            const int v = t >= off ? s_scan[t - off] : 0;
            const int u = RST && t >= off ? s_mark[t - off] : 0;
            __syncthreads();
            s_scan[t] += v;
            if (RST) s_mark[t] += u;
            __syncthreads();
        }
        const int first = carry + s_scan[t] - c;
        if (i < nsub) w.first[row + i] = first;
        if (RST && mk.n > 0) {  // this lane's first marker is the k-th of the scan
            const int64_t k = (int64_t)mcarry + s_mark[t] - mk.n;
            if ((int64_t)first + mk.first != (k + 1) * sc.restart_interval * sc.blocks_in_mcu || mk.idx != (int)(k & 7)) bad = 1;
        }
        if (RST && mk.bad) bad = 1;
        carry += s_scan[HT - 1];
        if (RST) mcarry += s_mark[HT - 1];
        __syncthreads();
    }
    const int any_bad = __syncthreads_or(bad);
    if (t == 0) {
        const State last = w.out[row + nsub - 1];
        bool ok = !any_bad && carry == total && last.pos == (uint32_t)len * 8u && last.bz == 0;
        if (RST && mcarry != (sc.mcus_w * sc.mcus_h - 1) / sc.restart_interval) ok = false;
        if (!ok) status[img] = LLFE_ERR_UNSUPPORTED;
    }
}

template <bool RST>
__global__ __launch_bounds__(HT) void k_huff_write(const uint8_t *__restrict__ staging,
                                                   const llfe_jpeg_scan *__restrict__ scans,
                                                   const llfe_jpeg_desc *__restrict__ descs, const int *__restrict__ status,
                                                   uint8_t *__restrict__ slots, int64_t slot_stride, Ws w) {
    __shared__ Shared S;
    const int img = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
    if (status[img] != 0 || (scans[img].restart_interval != 0) != RST) return;  // (whole workgroup)
    const int len = scans[img].scan_bytes, nsub = subsequences(len);
    if (g * HT >= nsub) return;  // (whole workgroup)
    load_shared(S, staging, &scans[img], &descs[img]);
    const llfe_jpeg_scan &sc = S.sc;
    const Tab *tabs = S.tabs;
    const uint8_t *nat = S.nat;
    const uint8_t *rec = staging + sc.record_offset;
    const int i = g * HT + t;
    if (i >= nsub) return;
    const Geometry geo{&sc, &S.d, slots + (int64_t)img * slot_stride};
    const int64_t lane = (int64_t)img * w.max_sub + i;
    const int total = sc.mcus_w * sc.mcus_h * sc.blocks_in_mcu;
    const int first = w.first[lane];
    if (first < 0 || first >= total) return;
    int cnt = 0;
    decode_sub<true, RST>(rec + sc.scan_offset, len, tabs, sc, w.in[lane], min(len, (i + 1) * kSub), &cnt, nat, geo,
                          w.dcd + (int64_t)img * w.max_blocks, first, total, nullptr);
}

template <bool RST>
__global__ __launch_bounds__(HT) void k_huff_dc(const uint8_t *__restrict__ staging,
                                                const llfe_jpeg_scan *__restrict__ scans,
                                                const llfe_jpeg_desc *__restrict__ descs, const int *__restrict__ status,
                                                uint8_t *__restrict__ slots, int64_t slot_stride, Ws w) {
    __shared__ int s_sum[3][HT];
    __shared__ int s_cut[RST ? HT : 1];  // RST: a sum restarted in or in front of this lane's MCUs
    __shared__ Shared S;
    const int img = blockIdx.x, t = threadIdx.x;
    if (status[img] != 0 || (scans[img].restart_interval != 0) != RST) return;  // (whole workgroup)
    load_shared(S, staging, &scans[img], &descs[img]);
    const llfe_jpeg_scan &sc = S.sc;
    const Geometry geo{&sc, &S.d, slots + (int64_t)img * slot_stride};
    const int16_t *dcd = w.dcd + (int64_t)img * w.max_blocks;
    const int bim = sc.blocks_in_mcu;
    const int64_t mcus = (int64_t)sc.mcus_w * sc.mcus_h;
    const int m0 = (int)(mcus * t / HT), m1 = (int)(mcus * (t + 1) / HT);  // this lane's MCUs
    // RST: the predictors are zero at every MCU m with m % Ri == 0, so a lane's sums are those
    // behind the last such MCU of its range, and the scan across the lanes is a segmented one
    const int ri = RST ? sc.restart_interval : 1;
    int sum0 = 0, sum1 = 0, sum2 = 0, cut = 0;
    for (int m = m0, left = RST ? m0 % ri : 0; m < m1; m++, left = left + 1 == ri ? 0 : left + 1)
        for (int b = 0; b < bim; b++) {
            if (RST && left == 0 && b == 0) sum0 = sum1 = sum2 = 0, cut = 1;
            const int c = sc.blk_comp[b], v = dcd[m * bim + b];
            sum0 += c == 0 ? v : 0;
            sum1 += c == 1 ? v : 0;
            sum2 += c == 2 ? v : 0;
        }
    s_sum[0][t] = sum0;
    s_sum[1][t] = sum1;
    s_sum[2][t] = sum2;
    if (RST) s_cut[t] = cut;
    __syncthreads();
    for (int off = 1; off < HT; off <<= 1) {
        int v[3];
        for (int c = 0; c < 3; c++) v[c] = t >= off ? s_sum[c][t - off] : 0;
        const int u = RST && t >= off ? s_cut[t - off] : 0;
        const bool open = !RST || !s_cut[t];  // nothing restarted yet in what this lane has summed
        __syncthreads();
        if (open) {
            for (int c = 0; c < 3; c++) s_sum[c][t] += v[c];
            if (RST) s_cut[t] = u;
        }
        __syncthreads();
    }
    int run0, run1, run2;  // exclusive
    if (RST) {
        run0 = t ? s_sum[0][t - 1] : 0, run1 = t ? s_sum[1][t - 1] : 0, run2 = t ? s_sum[2][t - 1] : 0;
    } else {
        run0 = s_sum[0][t] - sum0, run1 = s_sum[1][t] - sum1, run2 = s_sum[2][t] - sum2;
    }
    for (int m = m0, left = RST ? m0 % ri : 0; m < m1; m++, left = left + 1 == ri ? 0 : left + 1)
        for (int b = 0; b < bim; b++) {
            if (RST && left == 0 && b == 0) run0 = run1 = run2 = 0;
            const int blk = m * bim + b;
            int c;
            int16_t *dst = locate(geo, blk, &c);
            const int v = dcd[blk];
            run0 += c == 0 ? v : 0;
            run1 += c == 1 ? v : 0;
            run2 += c == 2 ? v : 0;
            if (dst) dst[0] = (int16_t)(c == 0 ? run0 : c == 1 ? run1 : run2);
        }
}

}  // namespace

size_t jpeg_huff_workspace_bytes(int n, int max_sub, int max_blocks) {
    size_t bytes = 0;
    carve(nullptr, n, max_sub, max_blocks, &bytes);
    return bytes;
}

int jpeg_huff_passes(int max_sub) { return (max_sub + HT - 1) / HT; }

template <bool RST>
static void launch_stage(int stage, int pass, const uint8_t *staging, const llfe_jpeg_scan *d_scans,
                         const llfe_jpeg_desc *d_descs, int n, uint8_t *slots, int64_t slot_stride, const Ws &w,
                         int *d_status, hipStream_t s) {
    const dim3 lanes((unsigned)w.max_wg, (unsigned)n);
    switch (stage) {
    case 1:
        hipLaunchKernelGGL(k_huff_sync<RST>, lanes, dim3(HT), 0, s, staging, d_scans, d_descs, d_status, w, n, pass);
        break;
    case 2:
        hipLaunchKernelGGL(k_huff_verify<RST>, dim3((unsigned)n), dim3(HT), 0, s, d_scans, d_status, w);
        break;
    case 3:
        hipLaunchKernelGGL(k_huff_write<RST>, lanes, dim3(HT), 0, s, staging, d_scans, d_descs, d_status, slots, slot_stride, w);
        break;
    default:
        hipLaunchKernelGGL(k_huff_dc<RST>, dim3((unsigned)n), dim3(HT), 0, s, staging, d_scans, d_descs, d_status, slots,
                           slot_stride, w);
        break;
    }
}

hipError_t launch_jpeg_huff(int stage, int pass, int kinds, const uint8_t *staging, const llfe_jpeg_scan *d_scans,
                            const llfe_jpeg_desc *d_descs, int n, int max_sub, int max_blocks, int64_t max_coef_bytes,
                            uint8_t *slots, int64_t slot_stride, uint8_t *workspace, int *d_status, hipStream_t s) {
    if (n <= 0 || max_sub <= 0 || max_blocks <= 0) return hipSuccess;
    size_t bytes = 0;
    const Ws w = carve(workspace, n, max_sub, max_blocks, &bytes);
    if (stage == 0) {
        const int64_t wgs = (max_coef_bytes / 16 + HT - 1) / HT;
        const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(wgs, 64)), (unsigned)n);
        hipLaunchKernelGGL(k_huff_init, grid, dim3(HT), 0, s, staging, d_scans, d_descs, slots, slot_stride);
    } else {
        if (kinds & 1) launch_stage<false>(stage, pass, staging, d_scans, d_descs, n, slots, slot_stride, w, d_status, s);
        if (kinds & 2) launch_stage<true>(stage, pass, staging, d_scans, d_descs, n, slots, slot_stride, w, d_status, s);
    }
    return hipGetLastError();
}

}  // namespace llfe
