// Private host header of libllfe.so's C ABI (include/llfe.h): the context and what the
// units that implement the entry points share.
//   llfe_context.cpp   context, settings, statistics
//   llfe_pipeline.cpp  the batch pipeline and the stage helpers
//   llfe_stages.cpp    the stage drop-ins
//   llfe_resize.cpp    PIL / cv2 resize and the text binary
//   llfe_decode.cpp    JPEG / PNG decode on the device
//   llfe_colors_images.cpp  llfe_process_images and the colours of a mixed-size batch in one pass
//   llfe_shapes_images.cpp  the shapes and shadows of a mixed-size batch in one pass
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/llfe.h"
#include "contours.h"
#include "llfe_internal.h"

namespace llfe_host {
using namespace llfe;

// ------------------------------------------------------------------ thread pool
class Pool {
  public:
    explicit Pool(int n) {
        for (int i = 0; i < n; i++) th_.emplace_back([this] { run(); });
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    int size() const { return (int)th_.size(); }
    // run f(i) for i in [0, n) on the pool (+ calling thread), wait for all
    void parallel_for(int n, const std::function<void(int, int)> &f) {
        if (n <= 0) return;
        std::atomic<int> next{0};
        int done = 0;  // guarded by m_: the waiter checks it under the same lock, so a
                       // completion can never slip between its check and its sleep
        int workers = std::min((int)th_.size(), n);
        auto job = [&](int wid) {
            for (int i; (i = next.fetch_add(1)) < n;) f(i, wid);
        };
        {
            std::lock_guard<std::mutex> g(m_);
            for (int w = 0; w < workers; w++)
                q_.push_back([&, w] {
                    job(w + 1);
                    std::lock_guard<std::mutex> g2(m_);
                    done++;
                    cv_done_.notify_all();
                });
        }
        cv_.notify_all();
        job(0);
        std::unique_lock<std::mutex> lk(m_);
        cv_done_.wait(lk, [&] { return done == workers; });
    }

  private:
    void run() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (stop_ && q_.empty()) return;
                f = std::move(q_.back());
                q_.pop_back();
            }
            f();
        }
    }
    std::vector<std::thread> th_;
    std::vector<std::function<void()>> q_;
    std::mutex m_;
    std::condition_variable cv_, cv_done_;
    bool stop_ = false;
};

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t count) {
        if (count <= n) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

template <typename T>
struct HostBuf {
    T *p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t count) {
        if (count <= n) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) n = count;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    ~HostBuf() { release(); }
};

// batches in flight at once (llfe_submit_batch; LLFE_INFLIGHT picks 2 or 3)
constexpr int kMaxSlots = 3;

// device workspace of one chunk in flight
struct Work {
    DevBuf<uint8_t> d_in, d_cls, d_sroot, d_tflag;  // d_tflag: the stencil's hysteresis tile flags
    bool tflag_valid = false;  // d_tflag belongs to the class map in d_cls (stencil_params)
    DevBuf<int8_t> d_noise, d_nfield;  // d_nfield: the launch's noise field (unique.hip)
    DevBuf<uint64_t> d_bits, d_ebits, d_pmom;  // d_pmom: the partitions' moments (KmeansCubes::moments)
    DevBuf<unsigned long long> d_shadow;
    DevBuf<int> d_order, d_parent, d_nroots, d_ftlist, d_ptlist;
    DevBuf<uint16_t> d_lab, d_roots;
    DevBuf<uint32_t> d_raw, d_keys, d_kscratch, d_pmeta, d_tstrong, d_segtab;  // d_segtab: k_uq_scatter's run table
    DevBuf<CubeEnt> d_segcubes, d_cubes;
    DevBuf<CellEnt> d_segcells, d_cells;
    DevBuf<SupEnt> d_sups;
    DevBuf<int32_t> d_ncubes, d_ncells, d_nsups;
    DevBuf<int64_t> d_nuniq;
    DevBuf<KmeansAttemptOut> d_att;
    int km_n = 0, km_colors = 0;  // images / n_colors of the last k-means launch (d_att)
    DevBuf<KmeansImageOut> d_kout;
    DevBuf<long long> d_index;  // per-image global indices of the chunk (llfe_batch.indices)
    // GPU contours (contours_gpu.hip); capacities grow when a pass overflows them
    DevBuf<uint64_t> d_ct_planes;
    DevBuf<CtComp> d_ct_comps;
    DevBuf<uint8_t> d_ct_acc;
    DevBuf<int2> d_ct_pts, d_ct_refs, d_ct_stage;
    DevBuf<CtCounters> d_ct_ctr;
    DevBuf<int> d_ct_info;
    DevBuf<llfe_shape> d_ct_shapes;
    CtCaps ct_min{0, 0, 0, 0};  // grown minimum capacities (0 = defaults)
    // llfe_font_detect (font.hip): per-image records, the region lists of a pass
    DevBuf<llfe_font_result> d_font_rec;
    DevBuf<int4> d_font_reg;
    DevBuf<uint64_t> d_fbits;  // LLFE_FEATURE_FONTS: the chunk's font bit rows (k_font_bits)
};

// hipEvent pairs around launches (enabled by llfe_set_profiling)
struct Profiler {
    struct Rec {
        int kid, slot;
        hipEvent_t a, b;
        double bytes;
    };
    struct Stat {
        std::string name;
        int64_t launches = 0;
        double ms = 0, bytes = 0;
    };
    bool on = false;
    static constexpr int kStageSlot = -3;  // records of the stage entry points (caller's stream)
    int cur_slot = 0;  // slot of the work being enqueued (records are collected per slot)
    std::vector<hipEvent_t> all, free_;
    std::vector<Rec> pending;
    std::vector<Stat> stats;
    // debug (LLFE_TIMELINE=file): every collected record's start / end in ms after `base`,
    // an event recorded when profiling was switched on (tools/debug/pipe_timeline.py)
    hipEvent_t base = nullptr;
    FILE *tl = nullptr;
    hipEvent_t ev() {
        if (free_.empty()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            all.push_back(e);
            return e;
        }
        hipEvent_t e = free_.back();
        free_.pop_back();
        return e;
    }
    int kid(const char *name) {
        for (size_t i = 0; i < stats.size(); i++)
            if (stats[i].name == name) return (int)i;
        stats.push_back(Stat{name});
        return (int)stats.size() - 1;
    }
    hipEvent_t begin(hipStream_t s) {
        if (!on) return nullptr;
        hipEvent_t a = ev();
        if (a) (void)hipEventRecord(a, s);
        return a;
    }
    void end(hipEvent_t a, hipStream_t s, const char *name, double bytes) {
        if (!on || !a) return;
        hipEvent_t b = ev();
        if (!b) {
            free_.push_back(a);
            return;
        }
        (void)hipEventRecord(b, s);
        pending.push_back(Rec{kid(name), cur_slot, a, b, bytes});
    }
    // records of slot `slot` (-1: every slot, -2: every record) whose end event has
    // completed; a record still pending keeps its events (a recycled event still in
    // flight would time a later launch wrongly)
    void collect(int slot = -1) {
        size_t keep = 0;
        for (size_t i = 0; i < pending.size(); i++) {
            Rec &r = pending[i];
            const bool mine = slot == -2 || (slot == -1 ? r.slot >= 0 : r.slot == slot);
            if (!mine || hipEventQuery(r.b) != hipSuccess) {
                pending[keep++] = r;
                continue;
            }
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
                stats[r.kid].launches++;
                stats[r.kid].ms += ms;
                stats[r.kid].bytes += r.bytes;
                float t0 = 0.f;
                if (tl && base && hipEventElapsedTime(&t0, base, r.a) == hipSuccess)
                    fprintf(tl, "%s %d %.4f %.4f\n", stats[r.kid].name.c_str(), r.slot, t0, t0 + ms);
            }
            free_.push_back(r.a);
            free_.push_back(r.b);
        }
        pending.resize(keep);
        if (tl) fflush(tl);
    }
    // bytes known only after the launch completed (k-means sweeps)
    void add_bytes(const char *name, double bytes) {
        if (on) stats[kid(name)].bytes += bytes;
    }
    void reset() {
        for (auto &r : pending) {
            free_.push_back(r.a);
            free_.push_back(r.b);
        }
        pending.clear();
        stats.clear();
    }
    ~Profiler() {
        for (auto e : all) (void)hipEventDestroy(e);
        if (base) (void)hipEventDestroy(base);
        if (tl) fclose(tl);
    }
};

// Tags the profiler records of a stage entry point's launches (caller's stream), so
// llfe_collect_batch never takes them for a slot's; the previous tag returns on exit.
struct StageSlotScope {
    Profiler &prof;
    const int prev;
    explicit StageSlotScope(Profiler &p) : prof(p), prev(p.cur_slot) { prof.cur_slot = Profiler::kStageSlot; }
    ~StageSlotScope() { prof.cur_slot = prev; }
};

// a submitted batch between llfe_submit_* and llfe_collect_batch
struct Pending {
    bool busy = false, done = false;
    llfe_batch b{};
    uint32_t features = 0;
    std::vector<llfe_image_result> res;
    std::vector<llfe_shape> shp;
    std::vector<int64_t> idx;  // llfe_submit_images: the images' global indices (b.indices)
    std::vector<llfe_font_result> fnt;  // LLFE_FEATURE_FONTS: the records (llfe_font_records)
};

struct HostSlot;

// Device side of one chunk in flight, indexed by q: llfe_process_batch runs every chunk on
// lane 0, a submitted ticket on the lane of its host slot.
struct Lane {
    Work W;
    hipStream_t stream = nullptr, col_stream = nullptr;  // col_stream: the colour path
    hipEvent_t stream_done = nullptr;
    // the mask / shadow D2H runs on the copy stream; W is not overwritten before the D2H
    // that last read it (into this host slot) has finished
    const HostSlot *mask_reader = nullptr;
};

// Host side of one chunk in flight, indexed by slot: the pinned results of a chunk, so the
// host can trace chunk c's contours while the GPU runs chunk c + 1 (llfe_process_batch
// alternates slots 0 and 1; a submitted ticket takes slot ticket % inflight_max).
struct HostSlot {
    HostBuf<uint64_t> h_bits;
    // GPU contours: per-image (components, ref base, contours, kept, shape base),
    // counters and shape records
    HostBuf<int> h_ct_info;
    HostBuf<CtCounters> h_ct_ctr;
    HostBuf<llfe_shape> h_ct_shapes;
    int64_t ct_shape_cap = 0;
    HostBuf<unsigned long long> h_shadow;
    HostBuf<KmeansImageOut> h_kout;
    // LLFE_FEATURE_FONTS: the records and counters of the chunk's font pass
    HostBuf<llfe_font_result> h_font_rec;
    HostBuf<CtCounters> h_font_ctr;
    hipEvent_t chunk_done = nullptr;
    hipEvent_t mask_done = nullptr;   // shapes/shadows results are on the host
    hipEvent_t mask_ready = nullptr;  // orders the mask D2H after the hysteresis kernels
    // recorded at enqueue: the contour mode, whether the font pass ran its contours on the GPU
    // (else finish_chunk takes the host path) and the image table the chunk was read through
    // (llfe_submit_images in place; null: packed)
    bool gpu_ct = false, font_gpu = false;
    const uint64_t *img_tab = nullptr;
    // llfe_submit_images: the gather table (n source addresses, n row pitches)
    HostBuf<uint64_t> h_gather;
    DevBuf<uint64_t> d_gather;
    Pending pending;  // asynchronous submissions (llfe_submit_batch / llfe_collect_batch)
};

}  // namespace llfe_host

struct llfe_ctx {
    int device = 0;
    std::string err;
    llfe_host::Pool *pool = nullptr;
    llfe_host::Profiler prof;
    double host_ct_ms = 0;       // llfe_host_contour_stats
    int64_t host_ct_images = 0;
    llfe::StencilParams sp{};
    // up to kMaxSlots batches in flight (llfe_submit_batch): device and host side
    llfe_host::Lane lanes[llfe_host::kMaxSlots];
    llfe_host::HostSlot slots[llfe_host::kMaxSlots];
    hipEvent_t start_ev = nullptr;
    int inflight_max = 2;  // slot = ticket % inflight_max
    bool any_inflight() const {
        for (const llfe_host::HostSlot &h : slots)
            if (h.pending.busy) return true;
        return false;
    }
    int64_t next_ticket = 0, next_collect = 0;
    llfe_host::DevBuf<uint8_t> d_rsz_tmp, d_rsz_src;
    llfe_host::DevBuf<uint8_t> d_ragged;       // llfe_process_images: one size group's packed images
    llfe_host::DevBuf<int8_t> d_ragged_noise;
    // the one-pass colours of llfe_process_images_flags: the staged images and host noise of a
    // pass (its own buffers: the size groups of the other features run beside it), then its
    // records and its work table
    llfe_host::DevBuf<uint8_t> d_color_stage;
    llfe_host::DevBuf<int8_t> d_color_noise;
    llfe_host::HostBuf<uint8_t> h_uq_tab;
    llfe_host::DevBuf<uint8_t> d_uq_tab;
    // the one-pass shapes / shadows of llfe_process_images_routes: the staged images of a pass,
    // then its records, work table and tile table
    llfe_host::DevBuf<uint8_t> d_shape_stage;
    llfe_host::HostBuf<uint8_t> h_shape_tab;
    llfe_host::DevBuf<uint8_t> d_shape_tab;
    llfe_host::DevBuf<int32_t> d_coef;
    // llfe_thumbnail_pil_images: the call's tables (pinned, then on the device) and the staging
    // workspace of one chunk of images
    llfe_host::HostBuf<uint8_t> h_thumb_tab;
    llfe_host::DevBuf<uint8_t> d_thumb_tab, d_thumb_ws;
    // llfe_preprocess_images / llfe_resize_cv_images: the same two of its own
    llfe_host::HostBuf<uint8_t> h_cvimg_tab;
    llfe_host::DevBuf<uint8_t> d_cvimg_tab, d_cvimg_ws;
    llfe_host::DevBuf<uint8_t> d_text;                  // llfe_text_binary: gray, then its upscale
    llfe_host::DevBuf<unsigned long long> d_text_hist;  // 256 bins + threshold + count of 255s
    // contours on the GPU (contours_gpu.hip) or on the host pool from the D2H'd mask
    // (default: the host pool runs them while the GPU is in k-means, which measured
    // faster on one MI355X; LLFE_CONTOURS=gpu or llfe_set_contour_mode switch)
    bool gpu_contours = false;
    hipEvent_t input_ready = nullptr, colour_done = nullptr;  // intra-chunk stream split
    bool concurrent = true;           // llfe_set_concurrency
    // host-input copies of successive chunks / batches are chained (h2d_done of the last
    // one): with two batches in flight, batch k + 1's H2D then starts after batch k's
    // instead of splitting PCIe with it, so batch k's kernels start at half the latency
    hipEvent_t h2d_done = nullptr;
    bool h2d_pending = false;
    // the mask / shadow D2H runs on its own stream so the colour stage starts right after
    // the hysteresis kernels (HostSlot::mask_ready, Lane::mask_reader)
    hipStream_t copy_stream = nullptr;
    llfe_host::HostBuf<llfe::KmeansImageOut> h_kout;
    // llfe_jpeg_entropy_decode: the validated descriptors (pinned, then on the device)
    llfe_host::HostBuf<llfe_jpeg_desc> h_jpeg_desc;
    llfe_host::DevBuf<llfe_jpeg_desc> d_jpeg_desc;
    // llfe_jpeg_reconstruct[_images]: the call's image records, then its (image, tile) work table
    llfe_host::HostBuf<uint8_t> h_jpeg_img_tab;
    llfe_host::DevBuf<uint8_t> d_jpeg_img_tab;
    // llfe_jpeg_entropy_decode: the validated scan records and the kernels' workspace
    // (subsequence states, block counts, DC differences)
    llfe_host::HostBuf<llfe_jpeg_scan> h_jpeg_scan;
    llfe_host::DevBuf<llfe_jpeg_scan> d_jpeg_scan;
    llfe_host::DevBuf<uint8_t> d_jpeg_huff_ws;
    // the call's HuffImage records, then its two work tables
    llfe_host::HostBuf<uint8_t> h_jpeg_huff_tab;
    llfe_host::DevBuf<uint8_t> d_jpeg_huff_tab;
    // llfe_png_decode_device: the validated descriptors
    llfe_host::HostBuf<llfe_png_desc> h_png_desc;
    llfe_host::DevBuf<llfe_png_desc> d_png_desc;
    // the per-image status of a device decode (JPEG entropy decode and PNG)
    llfe_host::HostBuf<int32_t> h_dec_status;
    llfe_host::DevBuf<int32_t> d_dec_status;
    llfe_host::Work *km_last = nullptr;  // workspace of the last k-means launch (llfe_kmeans_attempts)
    llfe_host::HostBuf<uint64_t> h_fbits;  // font bit rows of a chunk on the host path
    int64_t font_fallbacks = 0;  // font chunks whose contours ran on the host pool
    // llfe_font_records: the records of the last process call (font_owner = LLFE_LAST_CALL) or
    // the last collected ticket, valid until the next process / collect
    std::vector<llfe_font_result> font_recs;
    int64_t font_owner = LLFE_LAST_CALL;
    bool font_has = false;
    // per-thread host scratch
    std::vector<std::vector<int8_t>> work;
    std::vector<llfe::Contours> cont;
    std::vector<llfe::ShapeScratch> shs;
    std::vector<std::vector<llfe_shape>> img_shapes;
    std::vector<int32_t> img_ncont;
    int64_t host_fallbacks = 0;  // GPU-contour chunks traced on the host instead
    // llfe_set_contour_mode(LLFE_CONTOURS_GPU_FORCE_FALLBACK): every GPU-traced chunk is
    // redone on the host path (diagnostic: exercises the fallback)
    bool force_ct_fallback = false;

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

#define HIPCHK(ctx, expr)                                                                                   \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return (ctx)->fail(LLFE_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                                 __FILE__, __LINE__);                                       \
    } while (0)

// launch `expr` bracketed by profiler events (name, algorithmic HBM bytes)
#define TIMED(ctx, s, name, bytes, expr)                  \
    do {                                                  \
        hipEvent_t ev_a_ = (ctx)->prof.begin(s);          \
        HIPCHK(ctx, expr);                                \
        (ctx)->prof.end(ev_a_, s, name, (double)(bytes)); \
    } while (0)

namespace llfe_host {

// llfe_context.cpp
int chunk_for(int h, int w);  // images per device pass
double workspace_gb();        // LLFE_WORKSPACE_GB (default 24): the budget chunk_for divides
inline bool valid_dims(int n, int h, int w) { return n >= 0 && h > 0 && w > 0 && (int64_t)h * w < (1LL << 31); }

// llfe_pipeline.cpp: the stage helpers, shared by the pipeline and the stage drop-ins
int stage_enter(llfe_ctx *ctx, const char *fn);
int stage_input(llfe_ctx *ctx, Work &W, const llfe_batch *b, int i0, int n, const uint8_t **d_img, const int8_t **d_noise,
                hipStream_t s);
int chunk_index(llfe_ctx *ctx, Work &W, const llfe_batch *b, int i0, int n, hipStream_t s, ImgIndex *out);
int hyst_work(llfe_ctx *ctx, Work &W, int n, int h, int w, HystWork *out);
int stencil_params(llfe_ctx *ctx, Work &W, int n, int h, int w, hipStream_t s, StencilParams *sp);
int run_hysteresis_dilate(llfe_ctx *ctx, Work &W, int n, int h, int w, uint64_t *bits, uint8_t *mask_u8, hipStream_t s);
int run_contours(llfe_ctx *ctx, Work &W, int n, int h, int w, const uint64_t *bits, hipStream_t s, bool boxes = false);
int copy_contours(llfe_ctx *ctx, Work &W, int n, HostSlot &H, hipStream_t cs);
void grow_contour_caps(Work &W, int n, int h, int w, const CtCounters &ct);
int color_stage(llfe_ctx *ctx, Work &W, const uint8_t *img, const uint64_t *img_tab, const int8_t *noise, int n, int h,
                int w, uint64_t seed, ImgIndex index, bool contiguous_keys, hipStream_t s,
                const UqImages *ragged = nullptr);
int kmeans_stage(llfe_ctx *ctx, Work &W, const uint32_t *keys, int64_t key_stride, const int64_t *d_nuniq, int n,
                 int n_colors, uint64_t seed, ImgIndex index, const KmeansCubes &cubes, hipStream_t s);
void fill_palette(llfe_image_result &r);
void fill_color_result(const KmeansImageOut &k, llfe_image_result &r);
// Shape records of n images from their bit-packed dilated masks (hb, host) on the context's
// thread pool, into results[i0 ...] and the caller's shape array.  ragged (may be null): image i
// is ragged[i].height x width with its words at hb + ragged[i].word_offset; else every image is
// h x w, one behind the other.
void host_shapes_from_bits(llfe_ctx *ctx, const uint64_t *hb, int n, int h, int w, int i0, llfe_image_result *results,
                           llfe_shape *shapes, int64_t shape_capacity, int64_t &total_shapes,
                           const llfe_shape_image *ragged = nullptr);
int32_t shadow_level(uint64_t sum, uint64_t count);
// llfe_shapes_images.cpp: shapes and shadows of all images in one pass (LLFE_IMAGES_SHAPES_ONE_PASS),
// every other feature of `features` by size group afterwards; arguments and statuses as
// process_images_grouped
int process_images_shapes_one_pass(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                                   int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                                   llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                                   int64_t *shapes_needed, llfe_stream stream);
// llfe_process_images by size groups (llfe_colors_images.cpp holds the entry points)
int process_images_grouped(llfe_ctx *ctx, const llfe_image_desc *images, int32_t n, uint32_t features,
                           int32_t preprocessing, int32_t n_colors, uint64_t seed, int64_t index_base,
                           llfe_image_result *results, llfe_shape *shapes, int64_t shape_capacity,
                           int64_t *shapes_needed, llfe_stream stream);

}  // namespace llfe_host
