// The entropy half of a baseline JPEG decode on the device: the scan's bytes (staged by
// llfe_jpeg_parse_batch, jpeg_decode.cpp) -> exactly the coefficient slots that
// llfe_jpeg_read_coefs_batch writes on the host, for llfe_jpeg_reconstruct (jpeg_images.hip).
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
// whose record has restart_interval 0 and <true> for the others; each instance is launched on
// the records and the work table of its own images, and only when the batch has such images, so
// a batch without restart intervals runs the launches and the code it always ran.  With RST the lanes
// cross markers (jpeg_huff_core.h) and keep, next to the block count, the Marks of their last
// decode; k_huff_verify scans the marker counts along with the block counts and accepts an
// image only if no lane's Marks are bad, the first marker of every lane is the one its ordinal k
// asks for (FF D0 + (k & 7), behind exactly (k + 1) * Ri * blocks_in_mcu blocks) and the markers
// are (MCUs - 1) / Ri in all; the later markers of a lane are checked against its first one by
// the decode itself.  k_huff_dc restarts its sums at every interval (a segmented scan).
// Images of any sizes.  Nothing here assumes one size per batch: every image the host takes has a
// HuffImage record (llfe_internal.h) with the offset of its slot in the coefficient buffer and
// its first lane, first workgroup and first DC difference in the workspace -- prefix sums of the
// subsequence counts, the workgroup counts and the block counts (padding blocks included) over
// the call's images, so the workspace holds the sums, not images x the longest scan.  The lane
// kernels (k_huff_sync, k_huff_write) run over a work table of (record, workgroup of that image)
// entries, as k_jpeg_images runs over (image, tile) entries; k_huff_verify and k_huff_dc take one
// workgroup per record.  The records of the images without a restart interval come first and each
// kind has its own work table, so an instance is launched on its own images only.
// llfe_jpeg_entropy_decode (one size, slot i at i x slot_stride) and
// llfe_jpeg_entropy_decode_images (tight slots) build the same records and tables.
// Only the undecided suffix is launched.  After pass p workgroup p of an image is final (above),
// and the number of passes is the largest workgroup count of any image, so in a batch of mixed
// sizes most entries are final long before the last pass.  The work table is ordered by workgroup
// index (then record), and pass p launches only the entries with g >= p.  This is sound with the
// double-buffered boundary array: an entry g launched in pass p reads, in buffer p & 1, what
// g - 1 wrote in pass p - 1, and g - 1 >= p - 1 was launched then; an entry g < p is not launched
// and its lanes' states and the boundary it wrote in pass g stay as they are, which is what entry
// g + 1 read in pass g + 1, its last.
// Everything an image's lanes write lies in its own slot and its own part of the workspace.
// Every index derives from records and descriptors the host validated (validate_scans,
// check_jpeg_desc) or from records the host built from them; every loop has a bound that follows
// from the scan length.
#include "jpeg_huff_core.h"
#include "llfe_internal.h"

namespace llfe {
namespace {

using namespace llfe_huff;

constexpr int HT = kJpegHuffLanes;  // lanes (subsequences) per workgroup

__constant__ uint8_t c_nat[64] = {LLFE_JPEG_NATURAL_ORDER};

struct Ws {
    State *in, *out;   // per lane
    int *cnt, *first;  // per lane
    State *bnd;        // 2 x wgs: the last exit state of each workgroup, double-buffered
    int16_t *dcd;      // per block
    Marks *marks;      // per lane (RST)
    int wgs;
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// the workspace of a call: the sums of its images' lanes, workgroups and blocks
Ws carve(uint8_t *base, size_t lanes, size_t wgs, size_t blocks, size_t *bytes) {
    Ws w;
    w.wgs = (int)wgs;
    size_t o = 0;
    w.in = (State *)(base + o), o += up16(lanes * sizeof(State));
    w.out = (State *)(base + o), o += up16(lanes * sizeof(State));
    w.cnt = (int *)(base + o), o += up16(lanes * sizeof(int));
    w.first = (int *)(base + o), o += up16(lanes * sizeof(int));
    w.bnd = (State *)(base + o), o += up16(2 * wgs * sizeof(State));
    w.dcd = (int16_t *)(base + o), o += up16(blocks * sizeof(int16_t));
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
                                                  const HuffImage *__restrict__ recs, int per_image) {
    // per_image workgroups for every record
    const HuffImage &im = recs[blockIdx.x / per_image];
    const int bx = blockIdx.x % per_image;
    const llfe_jpeg_scan &sc = scans[im.img];
    const llfe_jpeg_desc &d = descs[im.img];
    uint8_t *slot = slots + im.slot_offset;
    const uint8_t *rec = staging + sc.record_offset;
    if (bx == 0 && (int)threadIdx.x < d.n_comp * 8) {
        const int c = threadIdx.x >> 3, j = threadIdx.x & 7;
        *(uint4 *)(slot + d.comp[c].quant_offset + j * 16) = *(const uint4 *)(rec + sc.quant_offset + c * 128 + j * 16);
    }
    for (int c = 0; c < d.n_comp; c++) {
        const int64_t vecs = (int64_t)d.comp[c].blocks_w * d.comp[c].blocks_h * 8;  // 16-byte stores
        uint4 *dst = (uint4 *)(slot + d.comp[c].coef_offset);
        for (int64_t k = (int64_t)bx * HT + threadIdx.x; k < vecs; k += (int64_t)per_image * HT)
            dst[k] = make_uint4(0, 0, 0, 0);
    }
}

template <bool RST>
__global__ __launch_bounds__(HT) void k_huff_sync(const uint8_t *__restrict__ staging,
                                                  const llfe_jpeg_scan *__restrict__ scans,
                                                  const llfe_jpeg_desc *__restrict__ descs,
                                                  const HuffImage *__restrict__ recs,
                                                  const HuffWork *__restrict__ work, Ws w, int pass) {
    __shared__ Shared S;
    __shared__ State lds_out[HT];
    const HuffWork wk = work[blockIdx.x];  // (the entries of this kind with g >= pass)
    const HuffImage &im = recs[wk.rec];
    const int img = im.img, g = wk.g, t = threadIdx.x;
    const int len = scans[img].scan_bytes, nsub = subsequences(len);
    if (g * HT >= nsub) return;  // (whole workgroup)
    load_shared(S, staging, &scans[img], &descs[img]);
    const llfe_jpeg_scan &sc = S.sc;
    const Tab *tabs = S.tabs;
    const uint8_t *nat = S.nat;
    const uint8_t *scan = staging + sc.record_offset + sc.scan_offset;
    const int i = g * HT + t;
    const bool act = i < nsub;
    const int64_t lane = (int64_t)im.lane0 + i;
    const int64_t wg = (int64_t)im.wg0 + g;
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
    if (g > 0 && pass > 0) before = w.bnd[(int64_t)(pass & 1) * w.wgs + wg - 1];
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
        if (t == HT - 1 || i == nsub - 1) w.bnd[(int64_t)((pass + 1) & 1) * w.wgs + wg] = out;
    }
}

template <bool RST>
__global__ __launch_bounds__(HT) void k_huff_verify(const llfe_jpeg_scan *__restrict__ scans, int *__restrict__ status,
                                                    const HuffImage *__restrict__ recs, Ws w) {
    __shared__ int s_scan[HT];
    __shared__ int s_mark[RST ? HT : 1];
    const HuffImage &im = recs[blockIdx.x];  // (the records of this kind)
    const int img = im.img, t = threadIdx.x;
    const llfe_jpeg_scan &sc = scans[img];
    const int len = sc.scan_bytes, nsub = subsequences(len);
    const int total = sc.mcus_w * sc.mcus_h * sc.blocks_in_mcu;
    const int64_t row = im.lane0;
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
                                                   uint8_t *__restrict__ slots, const HuffImage *__restrict__ recs,
                                                   const HuffWork *__restrict__ work, Ws w) {
    __shared__ Shared S;
    const HuffWork wk = work[blockIdx.x];  // (every entry of this kind)
    const HuffImage &im = recs[wk.rec];
    const int img = im.img, g = wk.g, t = threadIdx.x;
    if (status[img] != 0) return;  // (whole workgroup) the verification refused the image
    const int len = scans[img].scan_bytes, nsub = subsequences(len);
    if (g * HT >= nsub) return;  // (whole workgroup)
    load_shared(S, staging, &scans[img], &descs[img]);
    const llfe_jpeg_scan &sc = S.sc;
    const Tab *tabs = S.tabs;
    const uint8_t *nat = S.nat;
    const uint8_t *rec = staging + sc.record_offset;
    const int i = g * HT + t;
    if (i >= nsub) return;
    const Geometry geo{&sc, &S.d, slots + im.slot_offset};
    const int64_t lane = (int64_t)im.lane0 + i;
    const int total = sc.mcus_w * sc.mcus_h * sc.blocks_in_mcu;
    const int first = w.first[lane];
    if (first < 0 || first >= total) return;
    int cnt = 0;
    decode_sub<true, RST>(rec + sc.scan_offset, len, tabs, sc, w.in[lane], min(len, (i + 1) * kSub), &cnt, nat, geo,
                          w.dcd + im.dcd0, first, total, nullptr);
}

template <bool RST>
__global__ __launch_bounds__(HT) void k_huff_dc(const uint8_t *__restrict__ staging,
                                                const llfe_jpeg_scan *__restrict__ scans,
                                                const llfe_jpeg_desc *__restrict__ descs, const int *__restrict__ status,
                                                uint8_t *__restrict__ slots, const HuffImage *__restrict__ recs, Ws w) {
    __shared__ int s_sum[3][HT];
    __shared__ int s_cut[RST ? HT : 1];  // RST: a sum restarted in or in front of this lane's MCUs
    __shared__ Shared S;
    const HuffImage &im = recs[blockIdx.x];  // (the records of this kind)
    const int img = im.img, t = threadIdx.x;
    if (status[img] != 0) return;  // (whole workgroup) the verification refused the image
    load_shared(S, staging, &scans[img], &descs[img]);
    const llfe_jpeg_scan &sc = S.sc;
    const Geometry geo{&sc, &S.d, slots + im.slot_offset};
    const int16_t *dcd = w.dcd + im.dcd0;
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

size_t jpeg_huff_workspace_bytes(const HuffPlan &p) {
    size_t bytes = 0;
    carve(nullptr, (size_t)p.lanes, (size_t)p.wgs, (size_t)p.blocks, &bytes);
    return bytes;
}

template <bool RST>
static void launch_stage(int stage, int pass, int from, const HuffPlan &p, const uint8_t *staging,
                         const llfe_jpeg_scan *d_scans, const llfe_jpeg_desc *d_descs, uint8_t *slots, const Ws &w,
                         int *d_status, hipStream_t s) {
    const int k = RST ? 1 : 0;
    const HuffImage *mine = p.d_recs + (RST ? p.n_recs[0] : 0);
    switch (stage) {
    case 1:
        hipLaunchKernelGGL(k_huff_sync<RST>, dim3((unsigned)(p.n_work[k] - from)), dim3(HT), 0, s, staging, d_scans, d_descs,
                           p.d_recs, p.d_work[k] + from, w, pass);
        break;
    case 2:
        hipLaunchKernelGGL(k_huff_verify<RST>, dim3((unsigned)p.n_recs[k]), dim3(HT), 0, s, d_scans, d_status, mine, w);
        break;
    case 3:
        hipLaunchKernelGGL(k_huff_write<RST>, dim3((unsigned)p.n_work[k]), dim3(HT), 0, s, staging, d_scans, d_descs,
                           d_status, slots, p.d_recs, p.d_work[k], w);
        break;
    default:
        hipLaunchKernelGGL(k_huff_dc<RST>, dim3((unsigned)p.n_recs[k]), dim3(HT), 0, s, staging, d_scans, d_descs, d_status,
                           slots, mine, w);
        break;
    }
}

hipError_t launch_jpeg_huff(int stage, int pass, const int from[2], const HuffPlan &p, const uint8_t *staging,
                            const llfe_jpeg_scan *d_scans, const llfe_jpeg_desc *d_descs, uint8_t *slots,
                            uint8_t *workspace, int *d_status, hipStream_t s) {
    if (p.n_recs[0] + p.n_recs[1] <= 0) return hipSuccess;
    size_t bytes = 0;
    const Ws w = carve(workspace, (size_t)p.lanes, (size_t)p.wgs, (size_t)p.blocks, &bytes);
    if (stage == 0) {
        hipLaunchKernelGGL(k_huff_init, dim3((unsigned)((p.n_recs[0] + p.n_recs[1]) * p.init_wgs)), dim3(HT), 0, s, staging,
                           d_scans, d_descs, slots, p.d_recs, p.init_wgs);
    } else {
        const int none[2] = {0, 0};
        const int *f = stage == 1 ? from : none;
        if (p.n_work[0] - f[0] > 0) launch_stage<false>(stage, pass, f[0], p, staging, d_scans, d_descs, slots, w, d_status, s);
        if (p.n_work[1] - f[1] > 0) launch_stage<true>(stage, pass, f[1], p, staging, d_scans, d_descs, slots, w, d_status, s);
    }
    return hipGetLastError();
}

}  // namespace llfe
