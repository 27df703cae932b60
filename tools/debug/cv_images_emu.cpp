// Host emulation of csrc/cvresize_images.hip: the kernels compiled as C++, a workgroup as 256 host
// threads with a barrier, for AddressSanitizer / UBSan (a stand-alone program: nothing of it is
// loaded into Python or run on a GPU).  Plans and checks are the library's own
// (llfe_preprocess_images.cpp is included below).  tools/debug/cv_images_emu.py builds it, feeds it
// the cases of tests/preprocess_images_cases.py and compares the bytes with the oracle.
#include <algorithm>
#include <barrier>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
using std::max;
using std::min;
#include "llfe_ctx.h"

#undef __shared__
#define __shared__ static
#undef __launch_bounds__
#define __launch_bounds__(...)
struct Idx { unsigned x = 0; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<> *g_bar = nullptr;
#define __syncthreads() g_bar->arrive_and_wait()
static inline float __fadd_rn(float a, float b) { return a + b; }
static inline float __fmul_rn(float a, float b) { return a * b; }
static inline float __int_as_float(int v) { float f; std::memcpy(&f, &v, 4); return f; }
static void emu_launch(unsigned grid, const std::function<void()> &body) {
    std::barrier<> bar(256);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 256; t++)
        th.emplace_back([&, t] {
            threadIdx.x = t;
            for (unsigned b = 0; b < grid; b++) {
                blockIdx.x = b;
                body();
                g_bar->arrive_and_wait();
            }
        });
    for (auto &t : th) t.join();
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) emu_launch((grid).x, [&] { k(__VA_ARGS__); })
#define hipGetLastError() hipSuccess
#include "cvresize_images.hip"
#undef hipGetLastError
#include "llfe_preprocess_images.cpp"

// usage: emu h w oh ow interp srckind in.bin out.bin   (srckind 0 packed, 1 strided, 2 offset3)
int main(int argc, char **argv) {
    using namespace llfe;
    if (argc < 9) return 2;
    const int h = atoi(argv[1]), w = atoi(argv[2]), oh = atoi(argv[3]), ow = atoi(argv[4]), interp = atoi(argv[5]),
              kind = atoi(argv[6]);
    ImgPlan P;
    P.h = h, P.w = w, P.oh = oh, P.ow = ow, P.interp = interp;
    cv_images_plan_check(P);
    if (P.err) { printf("plan error: %s\n", P.err); return 3; }
    const size_t row = (size_t)w * 3, stride = kind == 1 ? row + 29 : row, lead = kind == 2 ? 3 : 0;
    const size_t src_bytes = lead + (size_t)(h - 1) * stride + row;
    uint8_t *src = (uint8_t *)malloc(src_bytes);  // exact size: ASan sees any byte outside the image
    memset(src, 77, src_bytes);
    FILE *f = fopen(argv[7], "rb");
    for (int y = 0; y < h; y++)
        if (fread(src + lead + (size_t)y * stride, 1, row, f) != row) return 4;
    fclose(f);
    uint8_t *dst = (uint8_t *)malloc((size_t)oh * ow * 3);
    memset(dst, 0xA5, (size_t)oh * ow * 3);
    std::vector<int32_t> tab(P.p.tab.begin(), P.p.tab.end());
    int32_t *dtab = (int32_t *)malloc(std::max<size_t>(tab.size(), 1) * 4);
    if (!tab.empty()) memcpy(dtab, tab.data(), tab.size() * 4);
    CvImgRec *r = (CvImgRec *)calloc(1, sizeof(CvImgRec));
    r->src = src + lead, r->src_stride = (int64_t)stride, r->dst = dst;
    r->h = h, r->w = w, r->oh = oh, r->ow = ow, r->kind = P.p.kind, r->fx = P.p.fx, r->fy = P.p.fy;
    r->ks = P.p.ks, r->xmax = P.p.xmax, r->x_vec = P.p.x_vec, r->xt = 0, r->yt = (int32_t)P.p.ytab_off;
    r->tile_h = P.tile_h, r->tiles_x = (ow + kCvTileW - 1) / kCvTileW, r->arm = P.arm;
    const int nw = r->tiles_x * ((oh + P.tile_h - 1) / P.tile_h);
    CvImgWork *wk = (CvImgWork *)malloc(sizeof(CvImgWork) * nw);
    for (int t = 0; t < nw; t++) wk[t] = CvImgWork{0, t};
    printf("kind %d tile_h %d arm %d work %d\n", (int)P.p.kind, P.tile_h, P.arm, nw);
    if (launch_cv_images(P.p.kind, r, wk, nw, dtab, nullptr) != hipSuccess) return 5;
    f = fopen(argv[8], "wb");
    fwrite(dst, 1, (size_t)oh * ow * 3, f);
    fclose(f);
    free(src), free(dst), free(dtab), free(r), free(wk);
    return 0;
}
