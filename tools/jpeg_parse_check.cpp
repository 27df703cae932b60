// Stand-alone memory check of the host half of the device entropy decode (llfe_jpeg_parse_batch)
// and of the kernels' host twin (llfe_jpeg_entropy_reference; csrc/jpeg_decode.cpp with
// csrc/jpeg_huff_core.h, the code the kernels compile): built with -fsanitize=address,undefined
// together with that one source file (tests/test_jpeg_parse_sanitized.py does), it reads the
// JPEG files named on the command line, parses each one into an exactly sized heap record and
// decodes it, by subsequences and in one piece, into an exactly sized heap slot -- so a write
// past the record or the slot, or a read of the bit reader past the staged scan, is a sanitizer
// report -- and compares the slot with the one llfe_jpeg_read_coefs_batch extracts.
// With --restarts in front of the files, parses with LLFE_JPEG_PARSE_RESTARTS
// (tests/test_jpeg_restart_sanitized.py).  Prints one line per file; exit status 0 when every call returned a documented status and
// every decoded slot equals the extracted one.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "llfe.h"

int llfe_jpeg_info_one(const uint8_t *data, size_t size, int32_t *w, int32_t *h, int *ncomp);

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
    uint8_t *p;
    explicit Aligned(size_t bytes) : p((uint8_t *)aligned_alloc(16, bytes)) { memset(p, 0xA5, bytes); }
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
    for (int a = restarts ? 2 : 1; a < argc; a++) {
        const std::vector<uint8_t> f = slurp(argv[a]);
        int32_t w = 0, h = 0;
        int nc = 0;
        const int irc = f.empty() ? LLFE_ERR_INVALID : llfe_jpeg_info_one(f.data(), f.size(), &w, &h, &nc);
        if (irc != LLFE_OK || w <= 0 || h <= 0) w = h = 8;  // still parsed, with a size it does not have
        const int64_t slot_bytes = llfe_jpeg_coef_slot_bytes(h, w);
        const int64_t stride = LLFE_JPEG_RECORD_HEADER + (((int64_t)f.size() + 15) & ~(int64_t)15) + 16;
        Aligned rec((size_t)stride);
        llfe_jpeg_desc d;
        llfe_jpeg_scan s;
        int32_t st = 1;
        const uint8_t *p = f.data();
        const uint64_t sz = f.size();
        const int rc = llfe_jpeg_parse_batch_flags(&p, &sz, 1, h, w, rec.p, stride, slot_bytes, &d, &s, &st, 1, flags);
        if (rc != st || !documented(st) || (st != LLFE_OK && (d.n_comp != 0 || s.blocks_in_mcu != 0))) bad++;
        int st_sub = LLFE_ERR_UNSUPPORTED, st_one = LLFE_ERR_UNSUPPORTED, st_host = 1, equal = -1;
        if (st == LLFE_OK) {
            Aligned sub((size_t)slot_bytes), one((size_t)slot_bytes), host((size_t)slot_bytes);
            llfe_jpeg_desc dh;
            if (llfe_jpeg_entropy_reference(rec.p, stride, &s, &d, 1, h, w, sub.p, slot_bytes, &st_sub, 0) != LLFE_OK) bad++;
            if (llfe_jpeg_entropy_reference(rec.p, stride, &s, &d, 1, h, w, one.p, slot_bytes, &st_one, 1) != LLFE_OK) bad++;
            llfe_jpeg_read_coefs_batch(&p, &sz, 1, h, w, host.p, slot_bytes, &dh, &st_host, 1);
            if (st_sub != st_one || !documented(st_sub)) bad++;
            if (st_sub == LLFE_OK) {  // what the twin accepts is what libjpeg extracts
                equal = st_host == LLFE_OK && !memcmp(&d, &dh, sizeof d) && same_extents(d, sub.p, host.p) &&
                        same_extents(d, one.p, host.p);
                if (!equal) bad++;
            }
            // a record one byte group short of the scan: handed back, nothing overruns
            Aligned tight((size_t)(stride - 32));
            llfe_jpeg_desc d2;
            llfe_jpeg_scan s2;
            int32_t st2 = 1;
            llfe_jpeg_parse_batch_flags(&p, &sz, 1, h, w, tight.p, stride - 32, slot_bytes, &d2, &s2, &st2, 1, flags);
            if (!documented(st2)) bad++;
        }
        printf("%s: %dx%d parse %d scan %d bytes decode %d / %d host %d equal %d\n", argv[a], w, h, st,
               st == LLFE_OK ? s.scan_bytes : 0, st_sub, st_one, st_host, equal);
    }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
