// C ABI of libllfe.so (include/llfe.h): the context, its settings and statistics, the
// device-pass size and the CPU-count rules.
#include <dlfcn.h>
#include <sched.h>

#include <cmath>

#include "llfe_ctx.h"

using namespace llfe_host;

namespace llfe_host {

// Images per device pass.  One pass per call when the workspace allows it: a bigger
// pass amortises the k-means launch's tail (its longest attempts run 100 Lloyd
// iterations) over more work (512 x 1080p per pass: +10 % images/s over 256).  The
// workspace is ~16 B per pixel + the 5 MB per-image partition cube and cell tables + the
// gathered cube / cell tables (<= 4 MiB + 1 MiB), held
// within LLFE_WORKSPACE_GB (default 24 GB of the 288 GB of HBM) PER IN-FLIGHT SLOT: every
// slot of llfe_set_inflight owns one such workspace, so depth 3 takes about 3x the budget.
double workspace_gb() {
    double gb = 24.0;
    if (const char *e = getenv("LLFE_WORKSPACE_GB"); e && atof(e) > 0) gb = atof(e);
    return gb;
}

int chunk_for(int h, int w) {
    const double gb = workspace_gb();
    const double P = (double)h * (double)w;
    const double cubes = std::min(P, (double)kMaxCubes), cells = std::min(cubes, (double)kParts * kCellsPerPart);
    const double per_image = 16.0 * P +  // keys, segments, class map, labels, masks
                             (double)kParts * (kCubesPerPart * sizeof(CubeEnt) + kCellsPerPart * sizeof(CellEnt)) +
                             cubes * sizeof(CubeEnt) + 2.0 * cells * sizeof(CellEnt);  // the gathered tables
    const double n = gb * 1e9 / per_image;
    return (int)std::max(1.0, std::min(n, (double)kMaxKmeansBatch));
}

}  // namespace llfe_host

namespace {

// CV_32F Gaussian kernel of getGaussianKernel(n, sigma<=0): bit-exact softdouble
// construction (sigma = 0.15 n + 0.35, normalised, centre = 1/sum) cast to float.
void gauss_kernel_f32(int n, float *out) {
    double sigma = (double)n * 0.15 + 0.35;
    double scale2 = -0.125 / (sigma * sigma);
    int n2 = (n - 1) / 2;
    double vals[32], sum = 0.0;
    for (int i = 0, x = 1 - n; i < n2; i++, x += 2) {
        vals[i] = std::exp((double)(x * x) * scale2);
        sum += vals[i];
    }
    sum = sum * 2.0 + 1.0;
    double mul = 1.0 / sum;
    for (int i = 0; i < n2; i++) out[i] = out[n - 1 - i] = (float)(vals[i] * mul);
    out[n2] = (float)(1.0 * mul);
}

// CPUs this process may run on: the affinity mask (sched_getaffinity), capped by a
// cgroup v2 cpu.max quota -- std::thread::hardware_concurrency() counts the whole node
int usable_cpus() {
    int n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::max(1u, std::thread::hardware_concurrency());
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[64] = {0};
        long long period = 0;
        if (fscanf(f, "%63s %lld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0) {
            const long long q = atoll(quota) / period;
            if (q >= 1 && q < n) n = (int)q;
        }
        fclose(f);
    }
    return std::max(1, n);
}

// host cores per GPU process: the rank's own share when placement.bind() pinned it to its
// GPU's NUMA node (LLFE_RANK_CPUS), else the usable cores shared by the LOCAL_WORLD_SIZE
// ranks torchrun starts on the node
int cores_per_process() {
    if (const char *rc = getenv("LLFE_RANK_CPUS"); rc && atoi(rc) > 0) return atoi(rc);
    int local = 1;
    if (const char *lw = getenv("LOCAL_WORLD_SIZE"); lw && atoi(lw) > 0) local = atoi(lw);
    return std::max(1, usable_cpus() / local);
}

int default_threads() {
    const char *e = getenv("LLFE_HOST_THREADS");
    if (e && atoi(e) > 0) return atoi(e);
    return std::max(1, std::min(cores_per_process(), 16));
}

// every event and every stream of the context, in the order llfe_init creates them
std::vector<hipEvent_t *> ctx_events(llfe_ctx *c) {
    std::vector<hipEvent_t *> evs = {&c->start_ev, &c->input_ready, &c->colour_done, &c->h2d_done};
    for (int i = 0; i < kMaxSlots; i++)
        for (hipEvent_t *e : {&c->slots[i].chunk_done, &c->slots[i].mask_done, &c->lanes[i].stream_done,
                              &c->slots[i].mask_ready})
            evs.push_back(e);
    return evs;
}

std::vector<hipStream_t *> ctx_streams(llfe_ctx *c) {
    std::vector<hipStream_t *> sts = {&c->copy_stream};
    for (Lane &L : c->lanes) {
        sts.push_back(&L.stream);
        sts.push_back(&L.col_stream);
    }
    return sts;
}

}  // namespace

extern "C" {

int llfe_abi_version(void) { return LLFE_ABI_VERSION; }

int llfe_default_host_threads(void) { return default_threads(); }

// path of the HIP runtime this library's HIP calls resolved to (dladdr of hipMalloc):
// a process must hold exactly one, shared with whatever produced its device pointers
// and stream handles (e.g. PyTorch-ROCm's torch/lib/libamdhip64.so)
const char *llfe_hip_runtime(void) {
    static std::string path;
    if (path.empty()) {
        Dl_info info{};
        hipError_t (*fn)(void **, size_t) = &hipMalloc;
        if (dladdr((void *)fn, &info) && info.dli_fname) path = info.dli_fname;
        else path = "?";
    }
    return path.c_str();
}

int llfe_init(int device, llfe_ctx **out) {
    if (!out) return LLFE_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return LLFE_ERR_HIP;
    if (device < 0 || device >= count) return LLFE_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return LLFE_ERR_HIP;
    llfe_ctx *c = new llfe_ctx();
    c->device = device;
    for (hipEvent_t *e : ctx_events(c))
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
            llfe_destroy(c);
            return LLFE_ERR_HIP;
        }
    // all streams at the default priority: a higher priority for the shapes streams or
    // for the colour streams measured neutral
    for (hipStream_t *st : ctx_streams(c))
        if (hipStreamCreateWithFlags(st, hipStreamNonBlocking) != hipSuccess) {
            llfe_destroy(c);
            return LLFE_ERR_HIP;
        }
    if (const char *fl = getenv("LLFE_INFLIGHT")) c->inflight_max = std::min(kMaxSlots, std::max(2, atoi(fl)));
    // contours on the host pool unless the process has too few host cores for them: a
    // "ui" 1080p image costs 0.28-0.36 ms of one core (round 3, llfe_host_contour_stats), so
    // 4 cores trace a 512-image 50 % ui step in ~23 ms, inside the ~28 ms GPU step (4 ranks on
    // 4 cores each: 19.3k images/s host vs 17.7k GPU contours, profiles/r3/multi/); below 4
    // the GPU path.  LLFE_CONTOURS=host / gpu overrides.
    c->gpu_contours = cores_per_process() < 4;
    if (const char *cm = getenv("LLFE_CONTOURS")) {
        if (!strcmp(cm, "gpu")) c->gpu_contours = true;
        if (!strcmp(cm, "host")) c->gpu_contours = false;
    }
    gauss_kernel_f32(11, c->sp.k11);
    {
        static const float kG11[11] = {LLFE_GAUSS11_F32};
        if (std::memcmp(kG11, c->sp.k11, sizeof(kG11)) != 0) {  // (an invariant of this build)
            std::fprintf(stderr, "llfe: getGaussianKernel(11) differs from the stencil's constants\n");
            llfe_destroy(c);
            return LLFE_ERR_UNSUPPORTED;
        }
    }
    c->pool = new Pool(default_threads() - 1);
    int nt = c->pool->size() + 1;
    c->work.resize(nt);
    c->cont.resize(nt);
    c->shs.resize(nt);
    *out = c;
    return LLFE_OK;
}

int llfe_destroy(llfe_ctx *ctx) {
    if (!ctx) return LLFE_OK;
    (void)hipSetDevice(ctx->device);
    for (hipStream_t *st : ctx_streams(ctx))
        if (*st) (void)hipStreamSynchronize(*st);
    for (hipEvent_t *e : ctx_events(ctx))
        if (*e) (void)hipEventDestroy(*e);
    for (hipStream_t *st : ctx_streams(ctx))
        if (*st) (void)hipStreamDestroy(*st);
    delete ctx->pool;
    delete ctx;  // DevBuf / HostBuf members free themselves
    return LLFE_OK;
}

const char *llfe_last_error(llfe_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int llfe_set_profiling(llfe_ctx *ctx, int enable) {
    if (!ctx) return LLFE_ERR_INVALID;
    if (enable) ctx->prof.reset();
    ctx->prof.on = enable != 0;
    if (enable) {
        if (const char *path = getenv("LLFE_TIMELINE")) {  // debug: absolute kernel intervals
            HIPCHK(ctx, hipSetDevice(ctx->device));
            if (!ctx->prof.base) HIPCHK(ctx, hipEventCreate(&ctx->prof.base));
            HIPCHK(ctx, hipEventRecord(ctx->prof.base, nullptr));
            HIPCHK(ctx, hipEventSynchronize(ctx->prof.base));
            if (!ctx->prof.tl) ctx->prof.tl = fopen(path, "a");
            if (ctx->prof.tl) fprintf(ctx->prof.tl, "# base\n");
        }
    }
    return LLFE_OK;
}

int llfe_set_contour_mode(llfe_ctx *ctx, int mode) {
    if (!ctx || (mode != LLFE_CONTOURS_HOST && mode != LLFE_CONTOURS_GPU && mode != LLFE_CONTOURS_GPU_FORCE_FALLBACK))
        return LLFE_ERR_INVALID;
    if (ctx->any_inflight())
        return ctx->fail(LLFE_ERR_INVALID, "llfe_set_contour_mode with submitted batches not yet collected");
    ctx->gpu_contours = mode != LLFE_CONTOURS_HOST;
    ctx->force_ct_fallback = mode == LLFE_CONTOURS_GPU_FORCE_FALLBACK;
    return LLFE_OK;
}

int llfe_get_contour_mode(llfe_ctx *ctx) {
    if (!ctx) return LLFE_ERR_INVALID;
    if (!ctx->gpu_contours) return LLFE_CONTOURS_HOST;
    return ctx->force_ct_fallback ? LLFE_CONTOURS_GPU_FORCE_FALLBACK : LLFE_CONTOURS_GPU;
}

int llfe_set_inflight(llfe_ctx *ctx, int32_t depth) {
    if (!ctx || depth < 2 || depth > kMaxSlots) return LLFE_ERR_INVALID;
    if (ctx->any_inflight())
        return ctx->fail(LLFE_ERR_INVALID, "llfe_set_inflight with submitted batches not yet collected");
    ctx->inflight_max = depth;
    return LLFE_OK;
}

int llfe_get_inflight(llfe_ctx *ctx) { return ctx ? ctx->inflight_max : LLFE_ERR_INVALID; }

int llfe_set_concurrency(llfe_ctx *ctx, int enable) {
    if (!ctx) return LLFE_ERR_INVALID;
    ctx->concurrent = enable != 0;
    return LLFE_OK;
}

int llfe_kernel_stats(llfe_ctx *ctx, llfe_kernel_stat *out, int32_t cap) {
    if (!ctx) return LLFE_ERR_INVALID;
    ctx->prof.collect(-2);  // every completed launch (stage entry points never wait on a slot)
    int n = (int)ctx->prof.stats.size();
    for (int i = 0; i < n && i < cap && out; i++) {
        const auto &st = ctx->prof.stats[i];
        std::memset(&out[i], 0, sizeof(llfe_kernel_stat));
        std::snprintf(out[i].name, sizeof(out[i].name), "%s", st.name.c_str());
        out[i].launches = st.launches;
        out[i].total_ms = st.ms;
        out[i].bytes = st.bytes;
    }
    return n;
}

int llfe_host_contour_stats(llfe_ctx *ctx, double *busy_ms, int64_t *images, int32_t *threads, int32_t reset) {
    if (!ctx) return LLFE_ERR_INVALID;
    if (busy_ms) *busy_ms = ctx->host_ct_ms;
    if (images) *images = ctx->host_ct_images;
    if (threads) *threads = ctx->pool ? ctx->pool->size() : 0;
    if (reset) {
        ctx->host_ct_ms = 0;
        ctx->host_ct_images = 0;
    }
    return LLFE_OK;
}

int llfe_batch_capacity(int32_t h, int32_t w) {
    if (!valid_dims(1, h, w)) return LLFE_ERR_INVALID;
    return chunk_for(h, w);
}

}  // extern "C"
