// The thread fan-out of the host batch entries (jpeg_decode.cpp, png_decode.cpp, which are also
// built on their own without the device code).  Plain C++, no HIP types.
#ifndef LLFE_HOST_FANOUT_H
#define LLFE_HOST_FANOUT_H
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <new>
#include <thread>
#include <vector>

#include "llfe.h"

namespace llfe {

// status[i] = one(i) for i in [0, n), on up to `threads` threads (the caller is one of them) that
// take the indices from one counter; a std::bad_alloc out of one(i) is LLFE_ERR_OOM for that i.
// The first non-zero status in index order, else LLFE_OK.
template <typename One>
int fan_out(int n, int threads, int32_t *status, One one) {
    const int nt = std::max(1, std::min(threads > 0 ? threads : 1, n));
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int i; (i = next.fetch_add(1)) < n;) {
            try {
                status[i] = one(i);
            } catch (const std::bad_alloc &) {
                status[i] = LLFE_ERR_OOM;
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    for (int i = 0; i < n; i++)
        if (status[i]) return status[i];
    return LLFE_OK;
}

}  // namespace llfe
#endif
