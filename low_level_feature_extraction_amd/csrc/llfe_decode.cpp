// C ABI of libllfe.so (include/llfe.h): image decode on the device -- JPEG reconstruction,
// JPEG entropy decode and PNG inflate / unfilter, each on the caller's stream.  Every entry
// point validates on the host, uploads its records through pinned buffers, runs its launches
// under the stage profiler tag and waits for the stream.
#include <algorithm>
#include <utility>
#include <vector>

#include "jpeg_huff_core.h"
#include "jpeg_images.h"
#include "jpeg_orient.h"
#include "llfe_ctx.h"
#include "png_inflate_core.h"

using namespace llfe_host;

namespace {

// room for n records in a pinned buffer and its device twin
template <typename T>
hipError_t ensure_records(HostBuf<T> &h, DevBuf<T> &d, int n) {
    const hipError_t e = h.ensure((size_t)n);
    return e != hipSuccess ? e : d.ensure((size_t)n);
}

// n validated records: copied into the pinned buffer and uploaded from there on s
template <typename T>
hipError_t upload_records(HostBuf<T> &h, DevBuf<T> &d, const T *src, int n, hipStream_t s) {
    std::memcpy(h.p, src, sizeof(T) * (size_t)n);
    return hipMemcpyAsync(d.p, h.p, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, s);
}

// the end of a decode: the per-image status back, the stream waited for (the pinned records
// and the workspace are free again), the launches' profiler records collected
int download_status(llfe_ctx *ctx, int32_t *status_out, int n, hipStream_t s) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_dec_status.p, ctx->d_dec_status.p, sizeof(int32_t) * (size_t)n,
                               hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    ctx->prof.collect(Profiler::kStageSlot);
    std::memcpy(status_out, ctx->h_dec_status.p, sizeof(int32_t) * (size_t)n);
    return LLFE_OK;
}

// What both entropy entry points do behind their host checks.  For the images with
// blocks_in_mcu != 0: the HuffImage records (those without a restart interval first; slot i at
// images[i].slot_offset, or at i x slot_stride when images is null) and per kind the work table
// ordered by workgroup index, then record, up through one pinned buffer in one copy; then the
// kernels and the status back.  Totals of lanes, blocks or work entries beyond an int32 are
// LLFE_ERR_CAPACITY, before any launch.
int run_jpeg_huff(llfe_ctx *ctx, const char *who, const uint8_t *staging, int64_t staging_bytes,
                  const llfe_jpeg_scan *scans, const llfe_jpeg_desc *descs, int n, const llfe_jpeg_image *images,
                  int64_t slot_stride, uint8_t *slots, int32_t *status_out, hipStream_t s) {
    using llfe::HuffImage;
    using llfe::HuffWork;
    constexpr int HT = llfe::kJpegHuffLanes;
    llfe::HuffPlan plan;
    std::vector<HuffImage> recs;
    std::vector<int> wgs_of;  // per record
    int64_t max_coef_bytes = 0;
    double coef_bytes = 0;
    try {
        for (int kind = 0; kind < 2; kind++)
            for (int i = 0; i < n; i++) {
                const llfe_jpeg_scan &sc = scans[i];
                if (sc.blocks_in_mcu == 0 || (sc.restart_interval != 0) != (kind == 1)) continue;
                const int64_t nsub = llfe_huff::subsequences(sc.scan_bytes), wgs = (nsub + HT - 1) / HT;
                HuffImage r;
                r.slot_offset = images ? images[i].slot_offset : (int64_t)i * slot_stride;
                r.img = i;
                r.lane0 = (int32_t)plan.lanes;
                r.wg0 = (int32_t)plan.wgs;
                r.dcd0 = (int32_t)plan.blocks;
                plan.lanes += nsub;
                plan.wgs += wgs;
                plan.blocks += (int64_t)sc.mcus_w * sc.mcus_h * sc.blocks_in_mcu;
                if (plan.lanes > 0x7fffffff || plan.blocks > 0x7fffffff)
                    return ctx->fail(LLFE_ERR_CAPACITY, "%s: more than 2^31 subsequences or blocks in one call", who);
                plan.n_recs[kind]++;
                plan.n_work[kind] += (int)wgs;
                plan.passes = std::max(plan.passes, (int)wgs);
                recs.push_back(r);
                wgs_of.push_back((int)wgs);
                for (int c = 0; c < descs[i].n_comp; c++) {
                    const int64_t b = (int64_t)descs[i].comp[c].blocks_w * descs[i].comp[c].blocks_h * 128;
                    max_coef_bytes = std::max(max_coef_bytes, b);
                    coef_bytes += (double)b;
                }
            }
        for (int i = 0; i < n; i++) status_out[i] = scans[i].blocks_in_mcu ? LLFE_OK : LLFE_ERR_UNSUPPORTED;
        if (recs.empty()) return LLFE_OK;
        plan.init_wgs = (int)std::max<int64_t>(1, std::min<int64_t>((max_coef_bytes / 16 + HT - 1) / HT, 64));
        if ((int64_t)recs.size() * plan.init_wgs > 0x7fffffff)
            return ctx->fail(LLFE_ERR_CAPACITY, "%s: %zu images in one call", who, recs.size());
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const size_t rec_bytes = (recs.size() * sizeof(HuffImage) + 15) & ~(size_t)15;
        const size_t tab_bytes = rec_bytes + (size_t)plan.wgs * sizeof(HuffWork);
        HIPCHK(ctx, ctx->h_jpeg_huff_tab.ensure(tab_bytes));
        HIPCHK(ctx, ctx->d_jpeg_huff_tab.ensure(tab_bytes));
        std::memcpy(ctx->h_jpeg_huff_tab.p, recs.data(), recs.size() * sizeof(HuffImage));
        // from[k][p]: the entries of kind k with a workgroup index below p
        std::vector<int> from[2];
        HuffWork *wk = (HuffWork *)(ctx->h_jpeg_huff_tab.p + rec_bytes);
        plan.d_recs = (const HuffImage *)ctx->d_jpeg_huff_tab.p;
        for (int kind = 0, r0 = 0, w0 = 0; kind < 2; r0 += plan.n_recs[kind], w0 += plan.n_work[kind], kind++) {
            plan.d_work[kind] = (const HuffWork *)(ctx->d_jpeg_huff_tab.p + rec_bytes) + w0;
            from[kind].assign((size_t)plan.passes + 1, plan.n_work[kind]);
            int k = 0;
            for (int g = 0; g < plan.passes; g++) {
                from[kind][(size_t)g] = k;
                for (int r = r0; r < r0 + plan.n_recs[kind]; r++)
                    if (g < wgs_of[(size_t)r]) wk[w0 + k++] = HuffWork{r, g};
            }
        }
        HIPCHK(ctx, ensure_records(ctx->h_jpeg_desc, ctx->d_jpeg_desc, n));
        HIPCHK(ctx, ensure_records(ctx->h_jpeg_scan, ctx->d_jpeg_scan, n));
        HIPCHK(ctx, ensure_records(ctx->h_dec_status, ctx->d_dec_status, n));
        HIPCHK(ctx, ctx->d_jpeg_huff_ws.ensure(jpeg_huff_workspace_bytes(plan)));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_jpeg_huff_tab.p, ctx->h_jpeg_huff_tab.p, tab_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, upload_records(ctx->h_jpeg_desc, ctx->d_jpeg_desc, descs, n, s));
        HIPCHK(ctx, upload_records(ctx->h_jpeg_scan, ctx->d_jpeg_scan, scans, n, s));
        HIPCHK(ctx, upload_records(ctx->h_dec_status, ctx->d_dec_status, (const int32_t *)status_out, n, s));
        auto launch = [&](int stage, int pass) {
            const int f[2] = {from[0][(size_t)pass], from[1][(size_t)pass]};
            return launch_jpeg_huff(stage, pass, f, plan, staging, ctx->d_jpeg_scan.p, ctx->d_jpeg_desc.p, slots,
                                    ctx->d_jpeg_huff_ws.p, ctx->d_dec_status.p, s);
        };
        {
            StageSlotScope tag(ctx->prof);
            TIMED(ctx, s, "k_huff_init", coef_bytes, launch(0, 0));
            // the cross-workgroup passes, fixed here from the scan lengths
            for (int p = 0; p < plan.passes; p++) TIMED(ctx, s, "k_huff_sync", (double)staging_bytes, launch(1, p));
            TIMED(ctx, s, "k_huff_verify", (double)plan.lanes * 20, launch(2, 0));
            TIMED(ctx, s, "k_huff_write", (double)staging_bytes + (double)plan.blocks * 2, launch(3, 0));
            TIMED(ctx, s, "k_huff_dc", (double)plan.blocks * 6, launch(4, 0));
        }
    } catch (const std::bad_alloc &) {
        return ctx->fail(LLFE_ERR_OOM, "%s: out of host memory", who);
    }
    return download_status(ctx, status_out, n, s);
}

// What both reconstruction entry points do behind their host checks, on records the caller built
// from what it validated: per orientation group the tile count and the bytes moved, the records
// and then the work table (one part per group: a launch is uniform) up through one pinned buffer
// in one copy, a launch per group present.  More than 2^31 tiles are LLFE_ERR_CAPACITY, before
// any launch.
int run_jpeg_images(llfe_ctx *ctx, const char *who, const uint8_t *coefs, const std::vector<llfe::JpegImageRec> &recs,
                    uint8_t *out, hipStream_t s) {
    using llfe::JpegImageRec;
    using llfe::JpegWork;
    int64_t group_work[llfe::kJpegOrientGroups] = {0, 0, 0};  // tiles per orientation group
    double group_bytes[llfe::kJpegOrientGroups] = {0, 0, 0};
    auto tiles_of = [](const JpegImageRec &r) {
        llfe::JpegTiling t;
        llfe::jpeg_tiling(r.d.sampling, &t);
        return (int64_t)r.tiles_x * ((r.h + t.th - 1) / t.th);
    };
    for (const JpegImageRec &r : recs) {
        const int g = llfe::jpeg_orient_group(r.orient);
        group_work[g] += tiles_of(r);
        for (int c = 0; c < r.d.n_comp; c++)
            group_bytes[g] += (double)r.d.comp[c].blocks_w * r.d.comp[c].blocks_h * 128 + 128;
        group_bytes[g] += (double)r.h * r.w * 3;  // (the same for both shapes)
    }
    const int64_t n_work = group_work[0] + group_work[1] + group_work[2];
    if (n_work > 0x7fffffff) return ctx->fail(LLFE_ERR_CAPACITY, "%s: %lld tiles in one call", who, (long long)n_work);
    if (recs.empty()) return LLFE_OK;
    try {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const size_t rec_bytes = (recs.size() * sizeof(JpegImageRec) + 15) & ~(size_t)15;
        const size_t tab_bytes = rec_bytes + (size_t)n_work * sizeof(JpegWork);
        HIPCHK(ctx, ctx->h_jpeg_img_tab.ensure(tab_bytes));
        HIPCHK(ctx, ctx->d_jpeg_img_tab.ensure(tab_bytes));
        std::memcpy(ctx->h_jpeg_img_tab.p, recs.data(), recs.size() * sizeof(JpegImageRec));
        JpegWork *wk = (JpegWork *)(ctx->h_jpeg_img_tab.p + rec_bytes);
        for (int g = 0; g < llfe::kJpegOrientGroups; g++) {
            if (group_work[g] == 0) continue;
            for (size_t k = 0; k < recs.size(); k++) {
                if (llfe::jpeg_orient_group(recs[k].orient) != g) continue;
                const int tiles = (int)tiles_of(recs[k]);
                for (int q = 0; q < tiles; q++) *wk++ = JpegWork{(int32_t)k, q};
            }
        }
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_jpeg_img_tab.p, ctx->h_jpeg_img_tab.p, tab_bytes, hipMemcpyHostToDevice, s));
        {
            StageSlotScope tag(ctx->prof);
            // coefficients and tables in, BGR out: no plane goes through memory
            static const char *const names[llfe::kJpegOrientGroups] = {"k_jpeg_images", "k_jpeg_images_mirrored",
                                                                       "k_jpeg_images_transposed"};
            const JpegWork *d_work = (const JpegWork *)(ctx->d_jpeg_img_tab.p + rec_bytes);
            for (int g = 0; g < llfe::kJpegOrientGroups; g++) {
                if (group_work[g] == 0) continue;
                TIMED(ctx, s, names[g], group_bytes[g],
                      llfe::launch_jpeg_images(coefs, (const JpegImageRec *)ctx->d_jpeg_img_tab.p, d_work,
                                               (int)group_work[g], out, g, s));
                d_work += group_work[g];
            }
        }
        HIPCHK(ctx, hipStreamSynchronize(s));  // (the pinned table is free again)
        ctx->prof.collect(Profiler::kStageSlot);
    } catch (const std::bad_alloc &) {
        return ctx->fail(LLFE_ERR_OOM, "%s: out of host memory", who);
    }
    return LLFE_OK;
}

}  // namespace

extern "C" {

int llfe_jpeg_reconstruct(llfe_ctx *ctx, const uint8_t *coefs, int64_t slot_stride, const llfe_jpeg_desc *descs,
                          int32_t n, int32_t h, int32_t w, uint8_t *out_bgr, llfe_stream stream) {
    if (!ctx) return LLFE_ERR_INVALID;
    if (!valid_dims(n, h, w) || h > 65535 || w > 65535 || (n && (!coefs || !descs || !out_bgr)) || slot_stride <= 0 ||
        (slot_stride & 15) || ((uintptr_t)coefs & 15))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_reconstruct: bad arguments (n=%d h=%d w=%d slot_stride=%lld)", n, h,
                         w, (long long)slot_stride);
    // nothing is launched on a descriptor the host check has not passed
    if (!llfe::check_jpeg_descs(descs, n, h, w, slot_stride))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_reconstruct: a descriptor points outside its slot or does not "
                                           "cover %dx%d", w, h);
    // one record per staged image; image i's slot and result lie where its index puts them
    std::vector<llfe::JpegImageRec> recs;
    try {
        llfe::JpegTiling t;
        recs.reserve((size_t)n);
        for (int i = 0; i < n; i++) {
            if (descs[i].n_comp == 0) continue;  // staged elsewhere: its place in out stays as it is
            llfe::jpeg_tiling(descs[i].sampling, &t);
            llfe::JpegImageRec r;
            r.d = descs[i];
            r.slot_offset = (int64_t)i * slot_stride;
            r.out_offset = (int64_t)i * h * w * 3;
            r.h = h;
            r.w = w;
            r.tiles_x = (w + t.tw - 1) / t.tw;
            // (the result is tightly packed: an image may start at any byte)
            r.vec = (w % 4 == 0 && ((uintptr_t)(out_bgr + r.out_offset) & 3) == 0) ? 1 : 0;
            r.orient = 1;
            recs.push_back(r);
        }
    } catch (const std::bad_alloc &) {
        return ctx->fail(LLFE_ERR_OOM, "llfe_jpeg_reconstruct: out of host memory");
    }
    return run_jpeg_images(ctx, "llfe_jpeg_reconstruct", coefs, recs, out_bgr, (hipStream_t)stream);
}

int llfe_jpeg_images_tiling(int32_t sampling, int32_t *tile_w, int32_t *tile_h) {
    llfe::JpegTiling t;
    if (!tile_w || !tile_h || !llfe::jpeg_tiling(sampling, &t)) return LLFE_ERR_INVALID;
    *tile_w = t.tw;
    *tile_h = t.th;
    return LLFE_OK;
}

int llfe_jpeg_reconstruct_images(llfe_ctx *ctx, const uint8_t *coefs, int64_t coefs_bytes, const llfe_jpeg_image *images,
                                 const llfe_jpeg_desc *descs, int32_t n, uint8_t *out, int64_t out_capacity,
                                 llfe_stream stream) {
    return llfe_jpeg_reconstruct_images_oriented(ctx, coefs, coefs_bytes, images, descs, nullptr, n, out, out_capacity,
                                                 stream);
}

int llfe_jpeg_reconstruct_images_oriented(llfe_ctx *ctx, const uint8_t *coefs, int64_t coefs_bytes,
                                          const llfe_jpeg_image *images, const llfe_jpeg_desc *descs,
                                          const uint8_t *orientation, int32_t n, uint8_t *out, int64_t out_capacity,
                                          llfe_stream stream) {
    using llfe::JpegImageRec;
    if (!ctx) return LLFE_ERR_INVALID;
    if (n < 0 || (n && (!coefs || !images || !descs || !out)) || coefs_bytes < 0 || out_capacity < 0 ||
        ((uintptr_t)coefs & 15))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_reconstruct_images: bad arguments (n=%d coefs_bytes=%lld "
                                           "out_capacity=%lld)", n, (long long)coefs_bytes, (long long)out_capacity);
    // nothing is launched on a record the host check has not passed
    std::vector<JpegImageRec> recs;
    std::vector<std::pair<int64_t, int64_t>> ranges;  // [begin, end) of every result
    int64_t out_end = 0;
    try {
        recs.reserve((size_t)n);
        ranges.reserve((size_t)n);
        for (int i = 0; i < n; i++) {
            const llfe_jpeg_desc &d = descs[i];
            if (d.n_comp == 0) continue;  // staged elsewhere: its place in out stays as it is
            const llfe_jpeg_image &m = images[i];
            const int o = orientation ? orientation[i] : 1;
            int64_t blocks = 0;
            llfe::JpegTiling t;
            if (m.height <= 0 || m.width <= 0 || m.height > 65535 || m.width > 65535 || m.slot_offset < 0 ||
                (m.slot_offset & 15) || m.slot_bytes <= 0 || (m.slot_bytes & 15) || m.slot_offset > coefs_bytes ||
                m.slot_bytes > coefs_bytes - m.slot_offset || m.out_offset < 0 || (m.out_offset & 15) ||
                !llfe::check_jpeg_desc(d, m.height, m.width, m.slot_bytes, &blocks) || !llfe::jpeg_tiling(d.sampling, &t))
                return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_reconstruct_images: image %d: a record or descriptor "
                                                   "points outside its slot, the coefficient buffer or does not "
                                                   "cover %dx%d", i, m.width, m.height);
            if (!llfe::jpeg_orient_valid(o))
                return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_reconstruct_images: image %d: orientation %d", i, o);
            JpegImageRec r;
            r.d = d;
            r.slot_offset = m.slot_offset;
            r.out_offset = m.out_offset;
            r.h = m.height;
            r.w = m.width;
            r.tiles_x = (m.width + t.tw - 1) / t.tw;
            // (the result's row length: the coded height for a transposed result)
            r.vec = (llfe::jpeg_orient_row(o, m.height, m.width) % 4 == 0 && ((uintptr_t)out & 3) == 0) ? 1 : 0;
            r.orient = o;
            recs.push_back(r);
            const int64_t px_bytes = (int64_t)m.height * m.width * 3;  // (the same for both shapes)
            ranges.emplace_back(m.out_offset, m.out_offset + px_bytes);
            out_end = std::max(out_end, m.out_offset + px_bytes);
        }
        std::sort(ranges.begin(), ranges.end());
        for (size_t k = 1; k < ranges.size(); k++)
            if (ranges[k].first < ranges[k - 1].second)
                return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_reconstruct_images: two results overlap in out");
        if (out_end > out_capacity)
            return ctx->fail(LLFE_ERR_CAPACITY, "llfe_jpeg_reconstruct_images: out holds %lld bytes, the results end at "
                                                "%lld", (long long)out_capacity, (long long)out_end);
    } catch (const std::bad_alloc &) {
        return ctx->fail(LLFE_ERR_OOM, "llfe_jpeg_reconstruct_images: out of host memory");
    }
    return run_jpeg_images(ctx, "llfe_jpeg_reconstruct_images", coefs, recs, out, (hipStream_t)stream);
}

int llfe_jpeg_entropy_decode(llfe_ctx *ctx, const uint8_t *staging, int64_t staging_bytes, const llfe_jpeg_scan *scans,
                             const llfe_jpeg_desc *descs, int32_t n, int32_t h, int32_t w, uint8_t *slots,
                             int64_t slot_stride, int32_t *status_out, llfe_stream stream) {
    if (!ctx) return LLFE_ERR_INVALID;
    if (!valid_dims(n, h, w) || h > 65535 || w > 65535 || n > 65535 ||
        (n && (!staging || !scans || !descs || !slots || !status_out)) || slot_stride <= 0 || (slot_stride & 15) ||
        ((uintptr_t)slots & 15) || staging_bytes < 0 || ((uintptr_t)staging & 15))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_entropy_decode: bad arguments (n=%d h=%d w=%d slot_stride=%lld)", n,
                         h, w, (long long)slot_stride);
    int max_sub = 0, max_blocks = 0;
    // nothing is launched on a descriptor or a record the host check has not passed
    if (!llfe::check_jpeg_descs(descs, n, h, w, slot_stride))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_entropy_decode: a descriptor points outside its slot or does not "
                                           "cover %dx%d", w, h);
    if (!llfe_huff::validate_scans(scans, descs, n, staging_bytes, &max_sub, &max_blocks))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_entropy_decode: a scan record points outside the staging buffer, "
                                           "its MCU geometry does not cover the block grids or its restart interval is "
                                           "not 0..65535");
    return run_jpeg_huff(ctx, "llfe_jpeg_entropy_decode", staging, staging_bytes, scans, descs, n, nullptr, slot_stride,
                         slots, status_out, (hipStream_t)stream);
}

int llfe_jpeg_entropy_decode_images(llfe_ctx *ctx, const uint8_t *staging, int64_t staging_bytes,
                                    const llfe_jpeg_scan *scans, const llfe_jpeg_desc *descs,
                                    const llfe_jpeg_image *images, int32_t n, uint8_t *slots, int64_t slots_bytes,
                                    int32_t *status_out, llfe_stream stream) {
    if (!ctx) return LLFE_ERR_INVALID;
    if (n < 0 || (n && (!staging || !scans || !descs || !images || !slots || !status_out)) || slots_bytes < 0 ||
        ((uintptr_t)slots & 15) || staging_bytes < 0 || ((uintptr_t)staging & 15))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_entropy_decode_images: bad arguments (n=%d staging_bytes=%lld "
                                           "slots_bytes=%lld)", n, (long long)staging_bytes, (long long)slots_bytes);
    // nothing is launched on a descriptor or a record the host check has not passed
    try {
        if (!llfe_huff::validate_scans_images(scans, descs, images, n, staging_bytes, slots_bytes))
            return ctx->fail(LLFE_ERR_INVALID, "llfe_jpeg_entropy_decode_images: a scan record points outside the "
                                               "staging buffer, a descriptor outside its slot, a slot outside the "
                                               "coefficient buffer or into another image's, or a geometry does not "
                                               "cover its image");
    } catch (const std::bad_alloc &) {
        return ctx->fail(LLFE_ERR_OOM, "llfe_jpeg_entropy_decode_images: out of host memory");
    }
    return run_jpeg_huff(ctx, "llfe_jpeg_entropy_decode_images", staging, staging_bytes, scans, descs, n, images, 0,
                         slots, status_out, (hipStream_t)stream);
}

int llfe_png_decode_device(llfe_ctx *ctx, const uint8_t *staging, int64_t staging_bytes, const llfe_png_desc *descs,
                           int32_t n, int32_t h, int32_t w, uint8_t *raw, int64_t raw_stride, uint8_t *out_bgr,
                           int32_t *status_out, llfe_stream stream) {
    if (!ctx) return LLFE_ERR_INVALID;
    if (!valid_dims(n, h, w) || n > 65535 || (n && (!staging || !descs || !raw || !out_bgr || !status_out)) ||
        raw_stride <= 0 || (raw_stride & 15) || ((uintptr_t)raw & 15) || staging_bytes < 0 || ((uintptr_t)staging & 15))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_png_decode_device: bad arguments (n=%d h=%d w=%d raw_stride=%lld)", n, h,
                         w, (long long)raw_stride);
    // nothing is launched on a descriptor the host check has not passed
    if (!llfe_png::validate_png_descs(descs, n, h, w, staging_bytes, raw_stride))
        return ctx->fail(LLFE_ERR_INVALID, "llfe_png_decode_device: a descriptor points outside the staging buffer or "
                                           "its geometry is not %dx%d at 3 or 4 bytes per pixel", w, h);
    int staged = 0;
    double in_bytes = 0, raw_bytes = 0;
    for (int i = 0; i < n; i++) {
        status_out[i] = descs[i].deflate_bytes ? LLFE_OK : LLFE_ERR_UNSUPPORTED;
        if (descs[i].deflate_bytes) {
            staged++;
            in_bytes += descs[i].deflate_bytes;
            raw_bytes += (double)descs[i].raw_bytes;
        }
    }
    if (staged == 0) return LLFE_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, ensure_records(ctx->h_png_desc, ctx->d_png_desc, n));
    HIPCHK(ctx, ensure_records(ctx->h_dec_status, ctx->d_dec_status, n));
    HIPCHK(ctx, upload_records(ctx->h_png_desc, ctx->d_png_desc, descs, n, s));
    HIPCHK(ctx, upload_records(ctx->h_dec_status, ctx->d_dec_status, (const int32_t *)status_out, n, s));
    auto launch = [&](int stage) {
        return launch_png_decode(stage, staging, ctx->d_png_desc.p, n, h, w, raw, raw_stride, out_bgr, ctx->d_dec_status.p,
                                 s);
    };
    {
        StageSlotScope tag(ctx->prof);
        TIMED(ctx, s, "k_png_inflate", in_bytes + raw_bytes, launch(0));
        TIMED(ctx, s, "k_png_unfilter_bgr", raw_bytes + (double)staged * h * w * 3, launch(1));
    }
    return download_status(ctx, status_out, n, s);
}

}  // extern "C"
