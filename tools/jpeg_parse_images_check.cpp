// Stand-alone memory check of the host half of the device entropy decode of a batch of images
// of any sizes (llfe_jpeg_records_layout, llfe_jpeg_parse_images) and of the kernels' host twin
// over tight slots (llfe_jpeg_entropy_reference_images; csrc/jpeg_decode.cpp with
// csrc/jpeg_huff_core.h, the code the kernels compile): built with -fsanitize=address,undefined
// together with that one source file (tests/test_jpeg_parse_images_sanitized.py does), it takes
// the files named on the command line, whatever their sizes, as one ragged batch: the image
// records from their headers (llfe_jpeg_layout_one, the JPEG half of llfe_jpeg_images_layout,
// which csrc/png_decode.cpp owns), the record offsets, the parse into one exactly sized heap
// staging buffer, the twin by subsequences and in one piece into exactly sized heap slots -- so a
// write past a record or a slot, or a read of the bit reader past a staged scan, is a sanitizer
// report -- and the comparison with what llfe_jpeg_read_coefs_images extracts.
// With --restarts in front of the files, parses with LLFE_JPEG_PARSE_RESTARTS.  Prints one line
// per file; exit status 0 when every call returned a documented status, every descriptor equals
// the extraction's and every decoded slot equals the extracted one.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "llfe.h"

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

struct Aligned {  // exactly `bytes`, 16-byte aligned
    uint8_t *p = nullptr;
    explicit Aligned(size_t bytes) {
        if (posix_memalign((void **)&p, 16, bytes ? bytes : 1)) abort();
        memset(p, 0xA5, bytes);
    }
    ~Aligned() { free(p); }
};

static bool same_extents(const llfe_jpeg_desc &d, const uint8_t *a, const uint8_t *b) {
    for (int c = 0; c < d.n_comp; c++) {
        const size_t bytes = (size_t)d.comp[c].blocks_w * d.comp[c].blocks_h * 128;
        if (memcmp(a + d.comp[c].quant_offset, b + d.comp[c].quant_offset, 128) ||
            memcmp(a + d.comp[c].coef_offset, b + d.comp[c].coef_offset, bytes))
            return false;
    }
    return true;
}

int main(int argc, char **argv) {
    int bad = 0;
    const bool restarts = argc > 1 && !strcmp(argv[1], "--restarts");
    const uint32_t flags = restarts ? LLFE_JPEG_PARSE_RESTARTS : 0u;
    const int first = restarts ? 2 : 1, n = argc - first;
    std::vector<std::vector<uint8_t>> files;
    std::vector<llfe_jpeg_image> images((size_t)n);
    std::vector<const uint8_t *> ptrs;
    std::vector<uint64_t> sizes;
    int64_t slots_bytes = 0;
    for (int i = 0; i < n; i++) {
        files.push_back(slurp(argv[first + i]));
        const std::vector<uint8_t> &f = files.back();
        llfe_jpeg_image &m = images[(size_t)i];
        memset(&m, 0, sizeof m);
        const int rc = llfe_jpeg_layout_one(f.data(), f.size(), &m.height, &m.width, &m.slot_bytes);
        if (!documented(rc)) bad++;
        if (rc != LLFE_OK) m.slot_bytes = 0;
        m.slot_offset = slots_bytes;
        slots_bytes += m.slot_bytes;
    }
    for (int i = 0; i < n; i++) ptrs.push_back(files[(size_t)i].data()), sizes.push_back(files[(size_t)i].size());
    std::vector<int64_t> offs((size_t)n, -1);
    int64_t staging_bytes = -1;
    if (llfe_jpeg_records_layout(sizes.data(), images.data(), n, offs.data(), &staging_bytes) != LLFE_OK) bad++;
    Aligned staging((size_t)staging_bytes);
    std::vector<llfe_jpeg_desc> descs((size_t)n), dh((size_t)n);
    std::vector<llfe_jpeg_scan> scans((size_t)n);
    std::vector<int32_t> st((size_t)n, 1), st_sub((size_t)n, 1), st_one((size_t)n, 1), st_host((size_t)n, 1);
    llfe_jpeg_parse_images(ptrs.data(), sizes.data(), n, images.data(), offs.data(), staging.p, staging_bytes, descs.data(),
                           scans.data(), st.data(), 3, flags);
    // a staging buffer one byte short is refused before any parse
    if (staging_bytes > 0) {
        std::vector<llfe_jpeg_desc> d2((size_t)n);
        std::vector<llfe_jpeg_scan> s2((size_t)n);
        std::vector<int32_t> st2((size_t)n, 1);
        Aligned tight((size_t)(staging_bytes - 1));
        if (llfe_jpeg_parse_images(ptrs.data(), sizes.data(), n, images.data(), offs.data(), tight.p, staging_bytes - 1,
                                   d2.data(), s2.data(), st2.data(), 1, flags) != LLFE_ERR_INVALID)
            bad++;
    }
    Aligned sub((size_t)slots_bytes), one((size_t)slots_bytes), host((size_t)slots_bytes);
    if (llfe_jpeg_entropy_reference_images(staging.p, staging_bytes, scans.data(), descs.data(), images.data(), n, sub.p,
                                           slots_bytes, st_sub.data(), 0) != LLFE_OK)
        bad++;
    if (llfe_jpeg_entropy_reference_images(staging.p, staging_bytes, scans.data(), descs.data(), images.data(), n, one.p,
                                           slots_bytes, st_one.data(), 1) != LLFE_OK)
        bad++;
    llfe_jpeg_read_coefs_images(ptrs.data(), sizes.data(), n, images.data(), host.p, slots_bytes, dh.data(), st_host.data(),
                                3);
    for (int i = 0; i < n; i++) {
        const size_t k = (size_t)i;
        const llfe_jpeg_image &m = images[k];
        int equal = -1;
        if (!documented(st[k]) || (st[k] != LLFE_OK && (descs[k].n_comp != 0 || scans[k].blocks_in_mcu != 0))) bad++;
        if (st_sub[k] != st_one[k] || !documented(st_sub[k]) || (st[k] != LLFE_OK && st_sub[k] != LLFE_ERR_UNSUPPORTED)) bad++;
        if (st[k] == LLFE_OK && st_sub[k] == LLFE_OK) {  // what the twin accepts is what libjpeg extracts
            equal = st_host[k] == LLFE_OK && !memcmp(&descs[k], &dh[k], sizeof dh[k]) &&
                    same_extents(descs[k], sub.p + m.slot_offset, host.p + m.slot_offset) &&
                    same_extents(descs[k], one.p + m.slot_offset, host.p + m.slot_offset);
            if (!equal) bad++;
        }
        printf("%s: %dx%d slot %lld record %lld parse %d scan %d bytes decode %d / %d host %d equal %d\n", argv[first + i],
               m.width, m.height, (long long)m.slot_bytes, (long long)offs[k], st[k], st[k] == LLFE_OK ? scans[k].scan_bytes : 0,
               st_sub[k], st_one[k], st_host[k], equal);
    }
    printf("ragged batch of %d: %lld staging bytes, %lld slot bytes\n", n, (long long)staging_bytes, (long long)slots_bytes);
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
