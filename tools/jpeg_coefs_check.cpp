// Stand-alone memory check of the coefficient extraction (llfe_jpeg_read_coefs_batch,
// csrc/jpeg_decode.cpp): built with -fsanitize=address,undefined together with that one
// source file (tests/test_jpeg_coefs_sanitized.py does), it reads the JPEG files named on
// the command line, extracts each one's coefficients into an exactly sized heap slot -- so
// a write past the slot, or a read past libjpeg's block rows, is a sanitizer report -- and
// then the files of the most common size once more as one batch on three threads, and all
// files, whatever their sizes, as one ragged batch (llfe_jpeg_read_coefs_images) into tight
// slots laid out from their headers in one exactly sized buffer.
// Prints one line per file; exit status 0 when every call returned a documented status.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "llfe.h"

int llfe_jpeg_info_one(const uint8_t *data, size_t size, int32_t *w, int32_t *h, int *ncomp);
int llfe_jpeg_layout_one(const uint8_t *data, size_t size, int32_t *h, int32_t *w, int64_t *slot_bytes);

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static bool documented(int rc) {
    return rc == LLFE_OK || rc == LLFE_ERR_UNSUPPORTED || rc == LLFE_ERR_INVALID || rc == LLFE_ERR_CAPACITY;
}

int main(int argc, char **argv) {
    std::vector<std::vector<uint8_t>> files;
    std::map<std::pair<int, int>, std::vector<int>> by_size;
    int bad = 0, extracted = 0;
    for (int a = 1; a < argc; a++) {
        files.push_back(slurp(argv[a]));
        const std::vector<uint8_t> &f = files.back();
        int32_t w = 0, h = 0;
        int nc = 0;
        const int irc = f.empty() ? LLFE_ERR_INVALID : llfe_jpeg_info_one(f.data(), f.size(), &w, &h, &nc);
        if (irc != LLFE_OK || w <= 0 || h <= 0) {
            printf("%s: header status %d\n", argv[a], irc);
            w = h = 8;  // still goes through the batch call, with a size it does not have
        }
        const int64_t stride = llfe_jpeg_coef_slot_bytes(h, w);
        std::vector<uint8_t> slot((size_t)stride);  // exactly the documented size
        llfe_jpeg_desc d;
        int32_t st = 1;
        const uint8_t *p = f.data();
        const uint64_t sz = f.size();
        const int rc = llfe_jpeg_read_coefs_batch(&p, &sz, 1, h, w, slot.data(), stride, &d, &st, 1);
        int64_t end = 0;
        for (int c = 0; c < d.n_comp; c++)
            end = std::max<int64_t>(end, d.comp[c].coef_offset + (int64_t)d.comp[c].blocks_w * d.comp[c].blocks_h * 128);
        printf("%s: %dx%d status %d components %d class %d extent %lld of %lld\n", argv[a], w, h, st, d.n_comp, d.sampling,
               (long long)end, (long long)stride);
        if (rc != st || !documented(st) || end > stride || (st != LLFE_OK && d.n_comp != 0)) bad++;
        extracted += st == LLFE_OK;
        // half a slot: a subsampled image still fits, a 4:4:4 one is handed back, nothing overruns
        const int64_t half = (stride / 2 + 15) & ~(int64_t)15;
        std::vector<uint8_t> small((size_t)half);
        llfe_jpeg_read_coefs_batch(&p, &sz, 1, h, w, small.data(), half, &d, &st, 1);
        if (!documented(st)) bad++;
        if (irc == LLFE_OK) by_size[{h, w}].push_back(a - 1);
    }
    const std::vector<int> *most = nullptr;
    std::pair<int, int> hw{0, 0};
    for (auto &kv : by_size)
        if (!most || kv.second.size() > most->size()) most = &kv.second, hw = kv.first;
    if (most) {
        const int n = (int)most->size();
        const int64_t stride = llfe_jpeg_coef_slot_bytes(hw.first, hw.second);
        std::vector<uint8_t> slots((size_t)stride * n);
        std::vector<llfe_jpeg_desc> descs((size_t)n);
        std::vector<int32_t> st((size_t)n, 1);
        std::vector<const uint8_t *> ptrs;
        std::vector<uint64_t> sizes;
        for (int i : *most) ptrs.push_back(files[(size_t)i].data()), sizes.push_back(files[(size_t)i].size());
        llfe_jpeg_read_coefs_batch(ptrs.data(), sizes.data(), n, hw.first, hw.second, slots.data(), stride, descs.data(),
                                   st.data(), 3);
        int ok = 0;
        for (int i = 0; i < n; i++) {
            ok += st[(size_t)i] == LLFE_OK;
            if (!documented(st[(size_t)i])) bad++;
        }
        printf("batch of %d at %dx%d on 3 threads: %d extracted\n", n, hw.second, hw.first, ok);
    }
    {  // every file in one ragged batch: the same files are extracted, none past its tight slot
        const int n = (int)files.size();
        std::vector<llfe_jpeg_image> images((size_t)n);
        std::vector<const uint8_t *> ptrs;
        std::vector<uint64_t> sizes;
        int64_t total = 0;
        for (int i = 0; i < n; i++) {
            const std::vector<uint8_t> &f = files[(size_t)i];
            llfe_jpeg_image &m = images[(size_t)i];
            memset(&m, 0, sizeof m);
            if (!documented(llfe_jpeg_layout_one(f.data(), f.size(), &m.height, &m.width, &m.slot_bytes))) bad++;
            m.slot_offset = total;
            total += m.slot_bytes;
            ptrs.push_back(f.data());
            sizes.push_back(f.size());
        }
        std::vector<uint8_t> slots((size_t)total);
        std::vector<llfe_jpeg_desc> descs((size_t)n);
        std::vector<int32_t> st((size_t)n, 1);
        llfe_jpeg_read_coefs_images(ptrs.data(), sizes.data(), n, images.data(), slots.data(), total, descs.data(),
                                    st.data(), 3);
        int ok = 0;
        for (int i = 0; i < n; i++) {
            ok += st[(size_t)i] == LLFE_OK;
            if (!documented(st[(size_t)i]) || (st[(size_t)i] != LLFE_OK && descs[(size_t)i].n_comp != 0)) bad++;
        }
        printf("ragged batch of %d on 3 threads: %d extracted into %lld bytes\n", n, ok, (long long)total);
        if (ok != extracted) bad++;
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
