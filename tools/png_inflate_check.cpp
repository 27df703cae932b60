// Memory check of the PNG staging and of the device decode's host twin, for a sanitizer build:
//   g++ -fsanitize=address,undefined tools/png_inflate_check.cpp csrc/png_decode.cpp -lz -ldl -lpthread
// (tests/test_png_inflate_sanitized.py).  Every file named on the command line is parsed at its
// own size into an exactly sized heap record (llfe_png_parse_batch), the record is moved into a
// heap block of just the bytes the validation asks for, and decoded into exactly sized raw and
// pixel buffers (llfe_png_decode_reference, the code the kernels of csrc/png_inflate.hip
// compile): a bit reader that left the staged stream, or a store outside raw or the image, is a
// sanitizer report.  Prints one line per file: parse status, decode status, and whether the
// pixels equal llfe_decode_png_batch's (-1: not compared); "ok" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "llfe.h"

// png_decode.cpp dispatches JPEGs to jpeg_decode.cpp, which this program does not link
int llfe_jpeg_info_one(const uint8_t *, size_t, int32_t *, int32_t *, int *) { return LLFE_ERR_UNSUPPORTED; }
bool llfe_jpeg_available() { return false; }
int llfe_jpeg_decode_one(const uint8_t *, size_t, int32_t, int32_t, uint8_t *) { return LLFE_ERR_UNSUPPORTED; }
int llfe_jpeg_layout_one(const uint8_t *, size_t, int32_t *, int32_t *, int64_t *) { return LLFE_ERR_UNSUPPORTED; }
int llfe_jpeg_layout_one_oriented(const uint8_t *, size_t, int32_t *, int32_t *, int64_t *, uint8_t *) {
    return LLFE_ERR_UNSUPPORTED;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        const std::vector<uint8_t> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        // (heap copies of the exact size: a read past the file is a report too)
        uint8_t *data = (uint8_t *)malloc(blob.size() ? blob.size() : 1);
        if (!blob.empty()) memcpy(data, blob.data(), blob.size());
        int32_t w = 0, h = 0;
        if (llfe_png_info(data, blob.size(), &w, &h) != LLFE_OK) w = h = 4;
        const int64_t stride = (int64_t)((blob.size() + 15) & ~(size_t)15) + 48;
        uint8_t *rec = (uint8_t *)malloc((size_t)stride);
        llfe_png_desc d = {};
        int32_t parse_rc = LLFE_ERR_INVALID, dec_rc = 1;
        const uint64_t size = blob.size();
        const uint8_t *ptr = data;
        llfe_png_parse_batch(&ptr, &size, 1, h, w, rec, stride, &d, &parse_rc, 1);  // (stride >= 48: the batch is taken)
        int equal = -1;
        if (parse_rc == LLFE_OK) {
            const int64_t need = (((int64_t)d.deflate_bytes + 15) & ~(int64_t)15) + 16;
            uint8_t *exact = (uint8_t *)malloc((size_t)need);
            memcpy(exact, rec + d.record_offset, (size_t)need);
            d.record_offset = 0;
            uint8_t *raw = (uint8_t *)malloc((size_t)d.raw_bytes);
            const size_t img = (size_t)h * w * 3;
            uint8_t *out = (uint8_t *)malloc(img), *ref = (uint8_t *)malloc(img);
            memset(out, 0, img);
            if (llfe_png_decode_reference(exact, need, &d, 1, h, w, raw, d.raw_bytes, out, &dec_rc) != LLFE_OK) dec_rc = 2;
            if (dec_rc == LLFE_OK) {
                int32_t host_rc = 0;
                llfe_decode_png_batch(&ptr, &size, 1, h, w, ref, &host_rc, 1);
                equal = host_rc == LLFE_OK && memcmp(out, ref, img) == 0;
            }
            free(exact);
            free(raw);
            free(out);
            free(ref);
        }
        printf("%s parse %d decode %d equal %d\n", argv[a], parse_rc, dec_rc, equal);
        free(rec);
        free(data);
    }
    printf("ok\n");
    return 0;
}
