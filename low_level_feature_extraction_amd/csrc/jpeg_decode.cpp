// Host JPEG decoding for the decode step in front of the hot path: cv2.imdecode(buf,
// IMREAD_COLOR) at app/services/analyze/utils.py:108-109 and
// app/services/analyze/image_processor.py:208-211.
//
// OpenCV decodes JPEG with libjpeg(-turbo): default (ISLOW) IDCT, fancy upsampling,
// output colour space JCS_EXT_BGR for 1- and 3-component images (grfmt_jpeg.cpp
// JpegDecoder::readData), so the BGR bytes are libjpeg's own colour conversion.  This
// file drives the system libjpeg-turbo (libjpeg.so.8, the same codec family OpenCV
// and Pillow bundle) through dlopen -- no headers are installed in the image, so the
// few API types used are declared below for the JPEG_LIB_VERSION 80 ABI.
// jpeg_CreateDecompress checks the struct size against the library's own, so a
// layout mismatch is reported as LLFE_ERR_UNSUPPORTED (the caller then falls back to
// Pillow), never as corrupted memory.
//
// Cases handed back to the caller (LLFE_ERR_UNSUPPORTED): 4-component (CMYK / YCCK)
// images (OpenCV converts those with its own CMYK formula) and images with an EXIF
// orientation other than 1 (imdecode applies the rotation; decode.py does it with
// Pillow's exif_transpose).  Corrupt data that libjpeg rejects is LLFE_ERR_INVALID.
//
// The second entry point, llfe_jpeg_read_coefs_batch, stops the same decode after its entropy
// half (jpeg_read_coefficients) and copies the quantised coefficients and quantisation tables
// out for the device reconstruction (jpeg_images.hip); it takes fewer files than the decoder
// above (no libjpeg warning, complete progressive scans, 4:4:4 / 4:2:2 / 4:2:0 / grey only)
// and hands the rest back with LLFE_ERR_UNSUPPORTED.  llfe_jpeg_read_coefs_images is the same
// extraction for images that each have their own size and tight slot (jpeg_images.hip), laid
// out from the headers alone by layout_one behind llfe_jpeg_images_layout (png_decode.cpp).
#include <dlfcn.h>
#include <setjmp.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_fanout.h"
#include "jpeg_desc_check.h"
#include "jpeg_huff_core.h"
#include "jpeg_orient.h"
#include "llfe.h"

namespace llfe_jpeg {

typedef int jboolean;  // libjpeg's `boolean`
typedef unsigned int JDIMENSION;
constexpr int kJpegLibVersion = 80;
constexpr int JCS_GRAYSCALE = 1, JCS_RGB = 2, JCS_YCbCr = 3, JCS_EXT_BGR = 8;

struct ErrorMgr {  // struct jpeg_error_mgr
    void (*error_exit)(void *cinfo);
    void (*emit_message)(void *cinfo, int msg_level);
    void (*output_message)(void *cinfo);
    void (*format_message)(void *cinfo, char *buffer);
    void (*reset_error_mgr)(void *cinfo);
    int msg_code;
    union {
        int i[8];
        char s[80];
    } msg_parm;
    int trace_level;
    long num_warnings;
    const char *const *jpeg_message_table;
    int last_jpeg_message;
    const char *const *addon_message_table;
    int first_addon_message;
    int last_addon_message;
};

struct Decompress {  // struct jpeg_decompress_struct, JPEG_LIB_VERSION 80
    ErrorMgr *err;
    void *mem, *progress, *client_data;
    jboolean is_decompressor;
    int global_state;
    void *src;
    JDIMENSION image_width, image_height;
    int num_components, jpeg_color_space, out_color_space;
    unsigned int scale_num, scale_denom;
    double output_gamma;
    jboolean buffered_image, raw_data_out;
    int dct_method;
    jboolean do_fancy_upsampling, do_block_smoothing, quantize_colors;
    int dither_mode;
    jboolean two_pass_quantize;
    int desired_number_of_colors;
    jboolean enable_1pass_quant, enable_external_quant, enable_2pass_quant;
    JDIMENSION output_width, output_height;
    int out_color_components, output_components, rec_outbuf_height, actual_number_of_colors;
    void *colormap;
    JDIMENSION output_scanline;
    int input_scan_number;
    JDIMENSION input_iMCU_row;
    int output_scan_number;
    JDIMENSION output_iMCU_row;
    void *coef_bits;
    void *quant_tbl_ptrs[4], *dc_huff_tbl_ptrs[4], *ac_huff_tbl_ptrs[4];
    int data_precision;
    void *comp_info;
    jboolean is_baseline, progressive_mode, arith_code;
    uint8_t arith_dc_L[16], arith_dc_U[16], arith_ac_K[16];
    unsigned int restart_interval;
    jboolean saw_JFIF_marker;
    uint8_t JFIF_major_version, JFIF_minor_version, density_unit;
    uint16_t X_density, Y_density;
    jboolean saw_Adobe_marker;
    uint8_t Adobe_transform;
    jboolean CCIR601_sampling;
    void *marker_list;
    int max_h_samp_factor, max_v_samp_factor, min_DCT_h_scaled_size, min_DCT_v_scaled_size;
    JDIMENSION total_iMCU_rows;
    void *sample_range_limit;
    int comps_in_scan;
    void *cur_comp_info[4];
    JDIMENSION MCUs_per_row, MCU_rows_in_scan;
    int blocks_in_MCU;
    int MCU_membership[10];
    int Ss, Se, Ah, Al;
    int block_size;
    const int *natural_order;
    int lim_Se;
    int unread_marker;
    void *master, *main, *coef, *post, *inputctl, *marker, *entropy, *idct, *upsample, *cconvert, *cquantize;
};

// ---- the coefficient path (llfe_jpeg_read_coefs_batch): what jpeg_read_coefficients hands out
struct QuantTbl {  // JQUANT_TBL: natural (not zigzag) order
    uint16_t quantval[64];
    jboolean sent_table;
};

struct ComponentInfo {  // jpeg_component_info, JPEG_LIB_VERSION 80
    int component_id, component_index, h_samp_factor, v_samp_factor, quant_tbl_no, dc_tbl_no, ac_tbl_no;
    JDIMENSION width_in_blocks, height_in_blocks;
    int DCT_h_scaled_size, DCT_v_scaled_size;
    JDIMENSION downsampled_width, downsampled_height;
    jboolean component_needed;
    int MCU_width, MCU_height, MCU_blocks, MCU_sample_width, last_col_width, last_row_height;
    QuantTbl *quant_table;
    void *dct_table;
};
static_assert(sizeof(ComponentInfo) == 96, "jpeg_component_info of the v8 ABI on LP64");

typedef int16_t (*BlockRow)[64];  // JBLOCKROW: a row of 64-coefficient blocks

struct MemoryMgr {  // struct jpeg_memory_mgr: the method table in front of its limits
    void *alloc_small, *alloc_large, *alloc_sarray, *alloc_barray, *request_virt_sarray, *request_virt_barray,
        *realize_virt_arrays, *access_virt_sarray;
    BlockRow *(*access_virt_barray)(void *cinfo, void *ptr, JDIMENSION start_row, JDIMENSION num_rows,
                                    jboolean writable);
    void *free_pool, *self_destruct;
    long max_memory_to_use, max_alloc_chunk;
};

struct Api {
    ErrorMgr *(*std_error)(ErrorMgr *) = nullptr;
    void (*create)(Decompress *, int, size_t) = nullptr;
    void (*destroy)(Decompress *) = nullptr;
    void (*mem_src)(Decompress *, const unsigned char *, unsigned long) = nullptr;
    int (*read_header)(Decompress *, jboolean) = nullptr;
    jboolean (*start)(Decompress *) = nullptr;
    JDIMENSION (*read_scanlines)(Decompress *, uint8_t **, JDIMENSION) = nullptr;
    jboolean (*finish)(Decompress *) = nullptr;
    void **(*read_coefficients)(Decompress *) = nullptr;  // -> jvirt_barray_ptr[num_components]
    bool ok = false;
    Api() {
        if (const char *off = getenv("LLFE_NO_LIBJPEG"); off && *off == '1') return;
        void *h = dlopen("libjpeg.so.8", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        std_error = (ErrorMgr * (*)(ErrorMgr *)) dlsym(h, "jpeg_std_error");
        create = (void (*)(Decompress *, int, size_t))dlsym(h, "jpeg_CreateDecompress");
        destroy = (void (*)(Decompress *))dlsym(h, "jpeg_destroy_decompress");
        mem_src = (void (*)(Decompress *, const unsigned char *, unsigned long))dlsym(h, "jpeg_mem_src");
        read_header = (int (*)(Decompress *, jboolean))dlsym(h, "jpeg_read_header");
        start = (jboolean(*)(Decompress *))dlsym(h, "jpeg_start_decompress");
        read_scanlines = (JDIMENSION(*)(Decompress *, uint8_t **, JDIMENSION))dlsym(h, "jpeg_read_scanlines");
        finish = (jboolean(*)(Decompress *))dlsym(h, "jpeg_finish_decompress");
        ok = std_error && create && destroy && mem_src && read_header && start && read_scanlines && finish;
        if (ok) ok = abi_matches();
        // the coefficient path only: its absence leaves the decoder above as it is
        read_coefficients = (void **(*)(Decompress *))dlsym(h, "jpeg_read_coefficients");
    }
    // jpeg_CreateDecompress rejects a JPEG_LIB_VERSION or struct size that differs from
    // the library's own (JERR_BAD_LIB_VERSION / JERR_BAD_STRUCT_SIZE): probed once, so a
    // mismatch disables this decoder instead of failing every image as "corrupt"
    bool abi_matches();
};
const Api &api() {
    static Api a;
    return a;
}

struct Err {
    ErrorMgr mgr;
    char pad[256];  // slack in case the library's error manager is larger than declared
    jmp_buf jb;
    int code;
};

void on_error(void *cinfo) {
    Err *e = (Err *)((Decompress *)cinfo)->err;
    e->code = LLFE_ERR_INVALID;
    longjmp(e->jb, 1);
}
void on_output(void *) {}  // warnings (e.g. "Corrupt JPEG data: premature end") are not errors

bool Api::abi_matches() {
    Decompress ci;
    Err err;
    memset(&ci, 0, sizeof ci);
    ci.err = std_error(&err.mgr);
    err.mgr.error_exit = on_error;
    err.mgr.output_message = on_output;
    if (setjmp(err.jb)) return false;
    create(&ci, kJpegLibVersion, sizeof(Decompress));
    destroy(&ci);
    return true;
}

inline uint16_t rd16(const uint8_t *p, bool le) { return le ? (uint16_t)(p[0] | p[1] << 8) : (uint16_t)(p[0] << 8 | p[1]); }
inline uint32_t rd32(const uint8_t *p, bool le) {
    return le ? (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24
              : (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

// EXIF orientation (tag 0x0112 of IFD0 in the first APP1 "Exif" segment), 1 if absent
int exif_orientation(const uint8_t *d, size_t n) {
    size_t p = 2;
    while (p + 4 <= n && d[p] == 0xFF) {
        const uint8_t m = d[p + 1];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) {
            p += 2;
            continue;
        }
        if (m == 0xDA || m == 0xD9) break;  // SOS / EOI: no more header segments
        const size_t len = (size_t)d[p + 2] << 8 | d[p + 3];
        if (len < 2 || p + 2 + len > n) break;
        const uint8_t *s = d + p + 4;
        const size_t sl = len - 2;
        if (m == 0xE1 && sl >= 14 && !memcmp(s, "Exif\0\0", 6)) {
            const uint8_t *t = s + 6;
            const size_t tl = sl - 6;
            const bool le = t[0] == 'I';
            if (!(t[0] == t[1] && (t[0] == 'I' || t[0] == 'M'))) return 1;
            const uint32_t ifd = rd32(t + 4, le);
            if ((size_t)ifd + 2 > tl) return 1;
            const int cnt = rd16(t + ifd, le);
            for (int k = 0; k < cnt; k++) {
                const size_t e = (size_t)ifd + 2 + 12 * (size_t)k;
                if (e + 12 > tl) break;
                if (rd16(t + e, le) == 0x0112) return rd16(t + e + 8, le);
            }
            return 1;
        }
        p += 2 + len;
    }
    return 1;
}

// what the coefficient and record paths take: no rotation, or (orient: LLFE_JPEG_ORIENT) one the
// device applies (jpeg_orient.h); *o receives the value, 1 where the file has none
bool orientation_taken(const uint8_t *d, size_t n, bool orient, int *o = nullptr) {
    const int v = exif_orientation(d, n);
    if (o) *o = v;
    return v == 1 || (orient && llfe::jpeg_orient_valid(v));
}

// header only (sizes); returns LLFE_OK / error code
int info(const uint8_t *data, size_t size, int32_t *w, int32_t *h, int *ncomp) {
    const Api &A = api();
    if (!A.ok) return LLFE_ERR_UNSUPPORTED;
    Decompress ci;
    Err err;
    memset(&ci, 0, sizeof ci);
    ci.err = A.std_error(&err.mgr);
    err.mgr.error_exit = on_error;
    err.mgr.output_message = on_output;
    err.code = 0;
    if (setjmp(err.jb)) {
        A.destroy(&ci);
        return err.code;
    }
    A.create(&ci, kJpegLibVersion, sizeof(Decompress));
    A.mem_src(&ci, data, (unsigned long)size);
    A.read_header(&ci, 1);
    *w = (int32_t)ci.image_width;
    *h = (int32_t)ci.image_height;
    *ncomp = ci.num_components;
    A.destroy(&ci);
    return LLFE_OK;
}

// full decode into out (h x w x 3 BGR); `rows` is caller scratch for row pointers
int decode(const uint8_t *data, size_t size, int32_t h, int32_t w, uint8_t *out, std::vector<uint8_t *> &rows) {
    const Api &A = api();
    if (!A.ok) return LLFE_ERR_UNSUPPORTED;
    if (exif_orientation(data, size) != 1) return LLFE_ERR_UNSUPPORTED;
    rows.resize((size_t)h);
    for (int32_t y = 0; y < h; y++) rows[(size_t)y] = out + (size_t)y * w * 3;
    uint8_t **rp = rows.data();
    Decompress ci;
    Err err;
    memset(&ci, 0, sizeof ci);
    ci.err = A.std_error(&err.mgr);
    err.mgr.error_exit = on_error;
    err.mgr.output_message = on_output;
    err.code = 0;
    volatile int rc = LLFE_OK;
    if (setjmp(err.jb)) {
        A.destroy(&ci);
        return err.code;
    }
    A.create(&ci, kJpegLibVersion, sizeof(Decompress));
    A.mem_src(&ci, data, (unsigned long)size);
    A.read_header(&ci, 1);
    if (ci.num_components != 1 && ci.num_components != 3) {
        rc = LLFE_ERR_UNSUPPORTED;
    } else if ((int32_t)ci.image_width != w || (int32_t)ci.image_height != h) {
        rc = LLFE_ERR_CAPACITY;
    } else {
        ci.out_color_space = JCS_EXT_BGR;  // grfmt_jpeg.cpp: JCS_EXT_BGR, 3 components
        ci.out_color_components = 3;
        A.start(&ci);
        if ((int32_t)ci.output_width != w || (int32_t)ci.output_height != h || ci.output_components != 3) {
            rc = LLFE_ERR_UNSUPPORTED;
        } else {
            while (ci.output_scanline < ci.output_height) {
                const JDIMENSION before = ci.output_scanline;
                A.read_scanlines(&ci, rp + before, ci.output_height - before);
                if (ci.output_scanline == before) break;
            }
            A.finish(&ci);
        }
    }
    A.destroy(&ci);
    return rc;
}

// ---- coefficients for the device reconstruction (jpeg_images.hip)
constexpr int64_t kQuantBytes = 3 * 128;  // three 64 x u16 tables lead the slot

inline int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

int64_t coef_slot_bytes(int32_t h, int32_t w) {  // 4:4:4: three components of ceil(h/8) x ceil(w/8) blocks
    return kQuantBytes + 3 * div_up(h, 8) * div_up(w, 8) * 128;
}

// what both staging paths take, decided from libjpeg's own header parse: 8-bit, greyscale or
// YCbCr with chroma 1x1 and luma 1x1 / 2x1 / 2x2, of the batch's size
int classify(const Decompress &ci, const ComponentInfo *comp, int32_t h, int32_t w, int *sampling) {
    const int nc = ci.num_components;
    if (ci.data_precision != 8 || !comp ||
        !((nc == 1 && ci.jpeg_color_space == JCS_GRAYSCALE) || (nc == 3 && ci.jpeg_color_space == JCS_YCbCr)))
        return LLFE_ERR_UNSUPPORTED;
    if ((int32_t)ci.image_width != w || (int32_t)ci.image_height != h) return LLFE_ERR_CAPACITY;
    if (nc == 1) {
        *sampling = LLFE_JPEG_GRAY;
        return LLFE_OK;
    }
    const int hs = comp[0].h_samp_factor, vs = comp[0].v_samp_factor;
    const bool chroma11 = comp[1].h_samp_factor == 1 && comp[1].v_samp_factor == 1 &&
                          comp[2].h_samp_factor == 1 && comp[2].v_samp_factor == 1;
    *sampling = !chroma11 ? 0 : hs == 1 && vs == 1 ? LLFE_JPEG_444 : hs == 2 && vs == 1 ? LLFE_JPEG_422 :
                hs == 2 && vs == 2 ? LLFE_JPEG_420 : 0;
    return *sampling ? LLFE_OK : LLFE_ERR_UNSUPPORTED;
}

// the descriptor of an eligible image: block grids and slot offsets.  need_qt: the components'
// quant_table pointers are set (they are once a scan has started).
int geometry(const ComponentInfo *comp, int nc, int sampling, int32_t h, int32_t w, int64_t slot_bytes, bool need_qt,
             llfe_jpeg_desc *out) {
    llfe_jpeg_desc &d = *out;
    d.n_comp = nc;
    d.sampling = sampling;
    int64_t off = kQuantBytes;
    for (int c = 0; c < nc; c++) {
        const ComponentInfo &k = comp[c];
        const int hs = c ? (sampling == LLFE_JPEG_422 || sampling == LLFE_JPEG_420 ? 2 : 1) : 1;
        const int vs = c ? (sampling == LLFE_JPEG_420 ? 2 : 1) : 1;
        // the geometry the device pass assumes, checked against the library's own
        if ((need_qt && !k.quant_table) || (int64_t)k.downsampled_width != div_up(w, hs) ||
            (int64_t)k.downsampled_height != div_up(h, vs) ||
            (int64_t)k.width_in_blocks != div_up(k.downsampled_width, 8) ||
            (int64_t)k.height_in_blocks != div_up(k.downsampled_height, 8))
            return LLFE_ERR_UNSUPPORTED;
        d.comp[c].blocks_w = (int32_t)k.width_in_blocks;
        d.comp[c].blocks_h = (int32_t)k.height_in_blocks;
        d.comp[c].width = (int32_t)k.downsampled_width;
        d.comp[c].height = (int32_t)k.downsampled_height;
        d.comp[c].quant_offset = 128 * c;
        d.comp[c].coef_offset = off;
        off += (int64_t)k.width_in_blocks * k.height_in_blocks * 128;
    }
    // a caller may stage in slots smaller than the 4:4:4 worst case (a 4:2:0 feed needs half):
    // what does not fit is handed back like any other image this path does not take
    return off > slot_bytes ? LLFE_ERR_UNSUPPORTED : LLFE_OK;
}

// entropy-decode one image and copy its quantised coefficients and tables into `slot`.
// Every eligibility check comes before the first byte is written.
int read_coefs(const uint8_t *data, size_t size, int32_t h, int32_t w, uint8_t *slot, int64_t slot_bytes,
               llfe_jpeg_desc *desc, bool orient = false) {
    const Api &A = api();
    if (!A.ok || !A.read_coefficients) return LLFE_ERR_UNSUPPORTED;
    if (size < 3 || data[0] != 0xFF || data[1] != 0xD8 || data[2] != 0xFF) return LLFE_ERR_UNSUPPORTED;
    if (!orientation_taken(data, size, orient)) return LLFE_ERR_UNSUPPORTED;
    Decompress ci;
    Err err;
    memset(&ci, 0, sizeof ci);
    ci.err = A.std_error(&err.mgr);
    err.mgr.error_exit = on_error;
    err.mgr.output_message = on_output;
    err.code = 0;
    if (setjmp(err.jb)) {
        A.destroy(&ci);
        return err.code;
    }
    A.create(&ci, kJpegLibVersion, sizeof(Decompress));
    A.mem_src(&ci, data, (unsigned long)size);
    A.read_header(&ci, 1);
    const int nc = ci.num_components;
    const ComponentInfo *comp = (const ComponentInfo *)ci.comp_info;
    int sampling = 0;
    volatile int rc = classify(ci, comp, h, w, &sampling);
    void **arrays = nullptr;
    if (rc == LLFE_OK) {
        arrays = A.read_coefficients(&ci);  // every scan: the entropy half of the decode
        if (!arrays) rc = LLFE_ERR_INVALID;
        // a warning (a truncated scan, say) makes the library patch the image up in ways the
        // device pass does not restate
        else if (err.mgr.num_warnings != 0) rc = LLFE_ERR_UNSUPPORTED;
    }
    // a progressive file that ends before its last refinement scan is smoothed between blocks
    // by the decoder (do_block_smoothing): coef_bits holds the precision reached per coefficient
    if (rc == LLFE_OK && ci.progressive_mode && ci.coef_bits) {
        const int(*bits)[64] = (const int(*)[64])ci.coef_bits;
        for (int c = 0; c < nc; c++)
            for (int k = 0; k < 64; k++)
                if (bits[c][k] != 0) rc = LLFE_ERR_UNSUPPORTED;
    }
    llfe_jpeg_desc d;
    memset(&d, 0, sizeof d);
    if (rc == LLFE_OK) rc = geometry(comp, nc, sampling, h, w, slot_bytes, true, &d);
    if (rc == LLFE_OK) {
        const MemoryMgr *mem = (const MemoryMgr *)ci.mem;
        // (the table room a grey image leaves unused: a slot's bytes depend on the file alone)
        memset(slot + 128 * nc, 0, (size_t)(kQuantBytes - 128 * nc));
        for (int c = 0; c < nc; c++) {
            memcpy(slot + d.comp[c].quant_offset, comp[c].quant_table->quantval, 128);
            uint8_t *dst = slot + d.comp[c].coef_offset;
            const size_t row_bytes = (size_t)d.comp[c].blocks_w * 128;
            for (int32_t by = 0; by < d.comp[c].blocks_h; by++) {  // the real blocks, not the MCU padding
                BlockRow *rows = mem->access_virt_barray(&ci, arrays[c], (JDIMENSION)by, 1, 0);
                memcpy(dst + (size_t)by * row_bytes, rows[0], row_bytes);
            }
        }
        *desc = d;
    }
    A.destroy(&ci);
    return rc;
}

// llfe_jpeg_images_layout for one JPEG, headers only: its size (written once the header gave
// one, else 0 x 0) and, for a file read_coefs would take as far as its header tells, the tight
// bytes of its slot -- the end of its last component as geometry() lays a slot out, up to 16.
// orientation: NULL, or (LLFE_JPEG_ORIENT) where the EXIF orientation of a file that is taken goes
int layout_one(const uint8_t *data, size_t size, int32_t *h, int32_t *w, int64_t *slot_bytes, uint8_t *orientation) {
    *h = *w = 0;
    *slot_bytes = 0;
    if (orientation) *orientation = 1;
    const Api &A = api();
    if (!A.ok || !A.read_coefficients) return LLFE_ERR_UNSUPPORTED;
    if (size < 3 || data[0] != 0xFF || data[1] != 0xD8 || data[2] != 0xFF) return LLFE_ERR_UNSUPPORTED;
    Decompress ci;
    Err err;
    memset(&ci, 0, sizeof ci);
    ci.err = A.std_error(&err.mgr);
    err.mgr.error_exit = on_error;
    err.mgr.output_message = on_output;
    err.code = 0;
    if (setjmp(err.jb)) {
        A.destroy(&ci);
        return err.code;
    }
    A.create(&ci, kJpegLibVersion, sizeof(Decompress));
    A.mem_src(&ci, data, (unsigned long)size);
    A.read_header(&ci, 1);
    *w = (int32_t)ci.image_width;
    *h = (int32_t)ci.image_height;
    int sampling = 0;
    llfe_jpeg_desc d;
    memset(&d, 0, sizeof d);
    const ComponentInfo *comp = (const ComponentInfo *)ci.comp_info;
    int o = 1;
    volatile int rc = !orientation_taken(data, size, orientation != nullptr, &o) ? LLFE_ERR_UNSUPPORTED
                                                                                   : classify(ci, comp, *h, *w, &sampling);
    if (rc == LLFE_OK) rc = geometry(comp, ci.num_components, sampling, *h, *w, INT64_MAX, false, &d);
    if (rc == LLFE_OK) {
        const auto &k = d.comp[d.n_comp - 1];
        *slot_bytes = (k.coef_offset + (int64_t)k.blocks_w * k.blocks_h * 128 + 15) & ~(int64_t)15;
        if (orientation) *orientation = (uint8_t)o;
    }
    A.destroy(&ci);
    return rc;
}

// ---- the host half of the device entropy decode (jpeg_huff.hip): headers only
struct Dht {
    bool present = false;
    uint8_t counts[17] = {0};
    uint8_t vals[256] = {0};
};

// canonical codes of a DHT -> the decoder's table; false for an over-subscribed code (and, as
// libjpeg's jpeg_make_d_derived_tbl does, for one that uses the all-ones code of any length)
bool build_tab(const Dht &h, llfe_huff::Tab *t) {
    memset(t, 0, sizeof *t);
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        t->off[l] = k - (int)code;
        code += h.counts[l];
        k += h.counts[l];
        if (code >= (1u << l)) return false;
        t->lim[l] = code << (16 - l);
        code <<= 1;
    }
    t->lim[17] = t->lim[16];
    memcpy(t->vals, h.vals, 256);
    return k > 0 && k <= 256;
}

struct Walk {
    int nc = 0;
    uint8_t cid[3] = {0}, hv[3] = {0}, td[3] = {0}, ta[3] = {0};
    size_t scan_begin = 0, scan_end = 0;
    unsigned ri = 0;  // the last DRI in front of the scan
};

// The marker walk: one SOF0 / SOF1, the DHTs, exactly one SOS with every component and the
// whole spectrum, no restart interval, and the scan ending at an FF D9 that is the first marker
// after it.  restarts: a restart interval is taken too, and the scan of a file that has one may
// hold FF D0..D7 (where, is for the decoder to check).  Everything else is for another decoder.
int walk(const uint8_t *d, size_t n, Dht (&dht)[4], Walk &W, bool restarts) {
    size_t p = 2;
    bool sof = false;
    for (;;) {
        if (p + 4 > n || d[p] != 0xFF) return LLFE_ERR_UNSUPPORTED;
        const uint8_t m = d[p + 1];
        if (m == 0xFF || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return LLFE_ERR_UNSUPPORTED;
        const size_t len = (size_t)d[p + 2] << 8 | d[p + 3];
        if (len < 2 || p + 2 + len > n) return LLFE_ERR_UNSUPPORTED;
        const uint8_t *s = d + p + 4;
        const size_t sl = len - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (sof || sl < 6 || s[0] != 8) return LLFE_ERR_UNSUPPORTED;
            W.nc = s[5];
            if ((W.nc != 1 && W.nc != 3) || sl != 6 + 3 * (size_t)W.nc) return LLFE_ERR_UNSUPPORTED;
            for (int c = 0; c < W.nc; c++) {
                W.cid[c] = s[6 + 3 * c];
                W.hv[c] = s[7 + 3 * c];
            }
            sof = true;
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < sl) {
                const int cls = s[q] >> 4, id = s[q] & 15;
                if (cls > 1 || id > 1 || q + 17 > sl) return LLFE_ERR_UNSUPPORTED;
                Dht &t = dht[cls * 2 + id];
                t = Dht();
                size_t total = 0;
                for (int l = 1; l <= 16; l++) total += (t.counts[l] = s[q + l]);
                if (total > 256 || q + 17 + total > sl) return LLFE_ERR_UNSUPPORTED;
                memcpy(t.vals, s + q + 17, total);
                t.present = true;
                q += 17 + total;
            }
        } else if (m >= 0xC2 && m <= 0xCF) {  // progressive, lossless, arithmetic, DAC
            return LLFE_ERR_UNSUPPORTED;
        } else if (m == 0xDD) {
            if (sl != 2) return LLFE_ERR_UNSUPPORTED;
            W.ri = (unsigned)s[0] << 8 | s[1];
            if (W.ri && !restarts) return LLFE_ERR_UNSUPPORTED;  // a restart interval
        } else if (m == 0xDA) {
            if (!sof || sl < 1 || s[0] != W.nc || sl != 4 + 2 * (size_t)W.nc) return LLFE_ERR_UNSUPPORTED;
            for (int c = 0; c < W.nc; c++) {
                if (s[1 + 2 * c] != W.cid[c]) return LLFE_ERR_UNSUPPORTED;  // (frame order)
                W.td[c] = s[2 + 2 * c] >> 4;
                W.ta[c] = s[2 + 2 * c] & 15;
                if (W.td[c] > 1 || W.ta[c] > 1 || !dht[W.td[c]].present || !dht[2 + W.ta[c]].present)
                    return LLFE_ERR_UNSUPPORTED;
            }
            const uint8_t *e = s + 1 + 2 * W.nc;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return LLFE_ERR_UNSUPPORTED;
            W.scan_begin = p + 2 + len;
            size_t q = W.scan_begin;
            for (;;) {
                const uint8_t *f = q < n ? (const uint8_t *)memchr(d + q, 0xFF, n - q) : nullptr;
                if (!f || (size_t)(f - d) + 1 >= n) return LLFE_ERR_UNSUPPORTED;  // no EOI: truncated
                q = (size_t)(f - d);
                if (d[q + 1] == 0x00) {
                    q += 2;
                    continue;
                }
                if (W.ri && d[q + 1] >= 0xD0 && d[q + 1] <= 0xD7) {
                    q += 2;
                    continue;
                }
                if (d[q + 1] != 0xD9) return LLFE_ERR_UNSUPPORTED;  // RSTn without a DRI, another scan, fill bytes
                W.scan_end = q;
                return W.scan_end > W.scan_begin ? LLFE_OK : LLFE_ERR_UNSUPPORTED;
            }
        }
        p += 2 + len;
    }
}

// parse one image and stage its record; every eligibility check comes before the first byte is
// written
int parse_one(const uint8_t *data, size_t size, int32_t h, int32_t w, uint8_t *rec, int64_t record_offset,
              int64_t record_stride, int64_t slot_bytes, llfe_jpeg_desc *desc, llfe_jpeg_scan *scan, bool restarts,
              bool orient = false) {
    const Api &A = api();
    if (!A.ok) return LLFE_ERR_UNSUPPORTED;
    if (size < 3 || data[0] != 0xFF || data[1] != 0xD8 || data[2] != 0xFF) return LLFE_ERR_UNSUPPORTED;
    if (!orientation_taken(data, size, orient)) return LLFE_ERR_UNSUPPORTED;
    Decompress ci;
    Err err;
    memset(&ci, 0, sizeof ci);
    ci.err = A.std_error(&err.mgr);
    err.mgr.error_exit = on_error;
    err.mgr.output_message = on_output;
    err.code = 0;
    if (setjmp(err.jb)) {
        A.destroy(&ci);
        return err.code;
    }
    A.create(&ci, kJpegLibVersion, sizeof(Decompress));
    A.mem_src(&ci, data, (unsigned long)size);
    A.read_header(&ci, 1);
    const int nc = ci.num_components;
    const ComponentInfo *comp = (const ComponentInfo *)ci.comp_info;
    int sampling = 0;
    volatile int rc = classify(ci, comp, h, w, &sampling);
    if (rc == LLFE_OK && (ci.progressive_mode || ci.arith_code || (ci.restart_interval != 0 && !restarts) ||
                          ci.restart_interval > 65535 || err.mgr.num_warnings != 0))
        rc = LLFE_ERR_UNSUPPORTED;
    llfe_jpeg_desc d;
    memset(&d, 0, sizeof d);
    if (rc == LLFE_OK) rc = geometry(comp, nc, sampling, h, w, slot_bytes, false, &d);
    Dht dht[4];
    Walk W;
    if (rc == LLFE_OK) rc = walk(data, size, dht, W, restarts);
    const QuantTbl *qt[3] = {nullptr, nullptr, nullptr};
    if (rc == LLFE_OK) {  // this walk and the library's agree on the frame
        if (W.nc != nc || W.ri != ci.restart_interval) rc = LLFE_ERR_UNSUPPORTED;
        for (int c = 0; c < nc && rc == LLFE_OK; c++) {
            const ComponentInfo &k = comp[c];
            if (W.cid[c] != k.component_id || W.hv[c] != (k.h_samp_factor << 4 | k.v_samp_factor) || k.quant_tbl_no < 0 ||
                k.quant_tbl_no > 3 || !(qt[c] = (const QuantTbl *)ci.quant_tbl_ptrs[k.quant_tbl_no]))
                rc = LLFE_ERR_UNSUPPORTED;
        }
    }
    llfe_huff::Tab tabs[4];
    memset(tabs, 0, sizeof tabs);
    if (rc == LLFE_OK) {
        for (int c = 0; c < nc; c++)
            for (int t : {(int)W.td[c], 2 + (int)W.ta[c]})
                if (!build_tab(dht[t], &tabs[t])) rc = LLFE_ERR_UNSUPPORTED;
    }
    const int64_t scan_bytes = (int64_t)W.scan_end - (int64_t)W.scan_begin;
    const int64_t padded = ((scan_bytes + 15) & ~(int64_t)15) + 16;
    if (rc == LLFE_OK && (scan_bytes >= (1 << 28) || LLFE_JPEG_RECORD_HEADER + padded > record_stride))
        rc = LLFE_ERR_UNSUPPORTED;
    if (rc == LLFE_OK) {
        llfe_jpeg_scan s;
        memset(&s, 0, sizeof s);
        s.record_offset = record_offset;
        s.quant_offset = 0;
        s.table_offset = (int32_t)kQuantBytes;
        s.scan_offset = LLFE_JPEG_RECORD_HEADER;
        s.scan_bytes = (int32_t)scan_bytes;
        const int H = nc == 1 ? 1 : comp[0].h_samp_factor, V = nc == 1 ? 1 : comp[0].v_samp_factor;
        // a one-component scan is not interleaved: its MCU is one block and there is no padding
        s.mcus_w = nc == 1 ? d.comp[0].blocks_w : (int32_t)div_up(w, 8 * H);
        s.mcus_h = nc == 1 ? d.comp[0].blocks_h : (int32_t)div_up(h, 8 * V);
        int b = 0;
        for (int c = 0; c < nc; c++) {
            s.comp_hs[c] = (uint8_t)(c ? 1 : H);
            s.comp_vs[c] = (uint8_t)(c ? 1 : V);
            for (int y = 0; y < s.comp_vs[c]; y++)
                for (int x = 0; x < s.comp_hs[c]; x++, b++) {
                    s.blk_comp[b] = (uint8_t)c;
                    s.blk_x[b] = (uint8_t)x;
                    s.blk_y[b] = (uint8_t)y;
                    s.blk_dc[b] = W.td[c];
                    s.blk_ac[b] = W.ta[c];
                }
        }
        s.blocks_in_mcu = b;
        s.restart_interval = (int32_t)W.ri;
        memset(rec, 0, LLFE_JPEG_RECORD_HEADER);
        for (int c = 0; c < nc; c++) memcpy(rec + s.quant_offset + 128 * c, qt[c]->quantval, 128);
        memcpy(rec + s.table_offset, tabs, sizeof tabs);
        memcpy(rec + s.scan_offset, data + W.scan_begin, (size_t)scan_bytes);
        memset(rec + s.scan_offset + scan_bytes, 0, (size_t)(padded - scan_bytes));
        *desc = d;
        *scan = s;
    }
    A.destroy(&ci);
    return rc;
}

// the record of a file of `size` bytes in a ragged staging buffer (llfe_jpeg_records_layout)
inline int64_t record_bytes(uint64_t size) { return LLFE_JPEG_RECORD_HEADER + (((int64_t)size + 15) & ~(int64_t)15) + 16; }

// One image of llfe_jpeg_entropy_reference: the phases of jpeg_huff.hip, serially.  RST: the
// record has a restart interval.
template <bool RST>
int reference_one(const uint8_t *rec, const llfe_jpeg_scan &sc, const llfe_jpeg_desc &d, uint8_t *slot, bool one_piece) {
    using namespace llfe_huff;
    static const uint8_t nat[64] = {LLFE_JPEG_NATURAL_ORDER};
    const uint8_t *scan = rec + sc.scan_offset;
    const Tab *tabs = (const Tab *)(rec + sc.table_offset);
    const int len = sc.scan_bytes;
    const int total = sc.mcus_w * sc.mcus_h * sc.blocks_in_mcu;
    for (int c = 0; c < d.n_comp; c++) {  // phase 1
        memcpy(slot + d.comp[c].quant_offset, rec + sc.quant_offset + 128 * c, 128);
        memset(slot + d.comp[c].coef_offset, 0, (size_t)d.comp[c].blocks_w * d.comp[c].blocks_h * 128);
    }
    const int nsub = one_piece ? 1 : subsequences(len);
    auto end_of = [&](int i) { return one_piece ? len : std::min(len, (i + 1) * kSub); };
    const State start{0, 0};
    const Geometry g{&sc, &d, slot};
    std::vector<State> in((size_t)nsub), out((size_t)nsub), prev;
    std::vector<int> cnt((size_t)nsub, 0), first((size_t)nsub, 0);
    std::vector<Marks> marks((size_t)nsub, Marks{0, 0, 0, 0});
    for (int i = 0; i < nsub; i++) {  // phase 2: every lane from its guess ...
        in[i] = i ? State{sub_start<RST>(scan, len, i), 0} : start;
        out[i] = decode_sub<false, RST>(scan, len, tabs, sc, in[i], end_of(i), &cnt[i], nat, g, nullptr, 0, 0, &marks[i]);
    }
    for (int r = 0; r < nsub; r++) {  // ... then rounds from the predecessor's exit state
        prev = out;
        bool changed = false;
        for (int i = 1; i < nsub; i++)
            if (prev[i - 1].pos != kNone && !same(prev[i - 1], in[i])) {
                in[i] = prev[i - 1];
                out[i] = decode_sub<false, RST>(scan, len, tabs, sc, in[i], end_of(i), &cnt[i], nat, g, nullptr, 0, 0,
                                                &marks[i]);
                changed = true;
            }
        if (!changed) break;
    }
    int sum = 0;  // phases 3 and 4
    int64_t k = 0;  // RST: the markers in front of lane i
    for (int i = 0; i < nsub; i++) {
        if (out[i].pos == kNone || !same(in[i], i ? out[i - 1] : start)) return LLFE_ERR_UNSUPPORTED;
        first[i] = sum;
        const Marks &m = marks[(size_t)i];
        if (RST && (m.bad || (m.n > 0 && ((int64_t)sum + m.first != (k + 1) * sc.restart_interval * sc.blocks_in_mcu ||
                                          m.idx != (int)(k & 7)))))
            return LLFE_ERR_UNSUPPORTED;
        sum += cnt[i];
        k += m.n;
    }
    if (sum != total || out[nsub - 1].pos != (uint32_t)len * 8u || out[nsub - 1].bz != 0) return LLFE_ERR_UNSUPPORTED;
    if (RST && k != (sc.mcus_w * sc.mcus_h - 1) / sc.restart_interval) return LLFE_ERR_UNSUPPORTED;
    std::vector<int16_t> dcd((size_t)total, 0);
    for (int i = 0; i < nsub; i++) {  // phase 5
        int n = 0;
        decode_sub<true, RST>(scan, len, tabs, sc, in[i], end_of(i), &n, nat, g, dcd.data(), first[i], total, nullptr);
    }
    int dc[3] = {0, 0, 0};  // phase 6
    for (int blk = 0; blk < total; blk++) {
        int c;
        if (RST && blk % (sc.restart_interval * sc.blocks_in_mcu) == 0) dc[0] = dc[1] = dc[2] = 0;
        int16_t *dst = locate(g, blk, &c);
        dc[c] += dcd[(size_t)blk];
        if (dst) dst[0] = (int16_t)dc[c];
    }
    return LLFE_OK;
}

}  // namespace llfe_jpeg

// used by png_decode.cpp's format-dispatching batch decoder
bool llfe_jpeg_available() { return llfe_jpeg::api().ok; }

int llfe_jpeg_info_one(const uint8_t *data, size_t size, int32_t *w, int32_t *h, int *ncomp) {
    return llfe_jpeg::info(data, size, w, h, ncomp);
}
int llfe_jpeg_decode_one(const uint8_t *data, size_t size, int32_t h, int32_t w, uint8_t *out) {
    thread_local std::vector<uint8_t *> rows;
    const int rc = llfe_jpeg::decode(data, size, h, w, out, rows);
    if (rows.capacity() > (1u << 16)) std::vector<uint8_t *>().swap(rows);
    return rc;
}

extern "C" int64_t llfe_jpeg_coef_slot_bytes(int32_t height, int32_t width) {
    if (height <= 0 || width <= 0 || height > 65535 || width > 65535) return LLFE_ERR_INVALID;  // JPEG's own limit
    return llfe_jpeg::coef_slot_bytes(height, width);
}

extern "C" int llfe_jpeg_read_coefs_batch(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height,
                                          int32_t width, uint8_t *slots, int64_t slot_stride, llfe_jpeg_desc *descs,
                                          int32_t *status, int32_t threads) {
    if (n < 0 || (n && (!data || !sizes || !slots || !descs || !status)) || height <= 0 || width <= 0 ||
        height > 65535 || width > 65535 || slot_stride < 0)
        return LLFE_ERR_INVALID;
    return llfe::fan_out(n, threads, status, [&](int i) {
        memset(&descs[i], 0, sizeof descs[i]);  // n_comp 0: nothing staged for this image
        return data[i] ? llfe_jpeg::read_coefs(data[i], (size_t)sizes[i], height, width,
                                               slots + (size_t)i * (size_t)slot_stride, slot_stride, &descs[i])
                       : LLFE_ERR_INVALID;
    });
}

// used by png_decode.cpp's llfe_jpeg_images_layout (which owns the format dispatch and the pixel limit)
int llfe_jpeg_layout_one(const uint8_t *data, size_t size, int32_t *h, int32_t *w, int64_t *slot_bytes) {
    return llfe_jpeg::layout_one(data, size, h, w, slot_bytes, nullptr);
}
// the same with LLFE_JPEG_ORIENT (orientation not NULL: files with an EXIF orientation 2 .. 8 too)
int llfe_jpeg_layout_one_oriented(const uint8_t *data, size_t size, int32_t *h, int32_t *w, int64_t *slot_bytes,
                                  uint8_t *orientation) {
    return llfe_jpeg::layout_one(data, size, h, w, slot_bytes, orientation);
}

extern "C" int llfe_jpeg_orient_reference(const uint8_t *src_bgr, int32_t h, int32_t w, int32_t orientation,
                                          uint8_t *dst_bgr) {
    if (!src_bgr || !dst_bgr || h <= 0 || w <= 0 || !llfe::jpeg_orient_valid(orientation)) return LLFE_ERR_INVALID;
    const int64_t row = llfe::jpeg_orient_row(orientation, h, w);
    for (int32_t y = 0; y < h; y++)
        for (int32_t x = 0; x < w; x++) {
            int yr, xr;
            llfe::jpeg_orient_map(orientation, h, w, y, x, &yr, &xr);
            memcpy(dst_bgr + (yr * row + xr) * 3, src_bgr + ((int64_t)y * w + x) * 3, 3);
        }
    return LLFE_OK;
}

extern "C" int llfe_jpeg_read_coefs_images(const uint8_t *const *data, const uint64_t *sizes, int32_t n,
                                           const llfe_jpeg_image *images, uint8_t *slots, int64_t slots_bytes,
                                           llfe_jpeg_desc *descs, int32_t *status, int32_t threads) {
    return llfe_jpeg_read_coefs_images_flags(data, sizes, n, images, slots, slots_bytes, descs, status, threads, 0);
}

extern "C" int llfe_jpeg_read_coefs_images_flags(const uint8_t *const *data, const uint64_t *sizes, int32_t n,
                                                 const llfe_jpeg_image *images, uint8_t *slots, int64_t slots_bytes,
                                                 llfe_jpeg_desc *descs, int32_t *status, int32_t threads,
                                                 uint32_t flags) {
    if ((flags & ~LLFE_JPEG_ORIENT) || n < 0 || (n && (!data || !sizes || !images || !slots || !descs || !status)) ||
        slots_bytes < 0)
        return LLFE_ERR_INVALID;
    for (int i = 0; i < n; i++) {  // every slot inside the buffer, before the first byte is written
        const llfe_jpeg_image &m = images[i];
        if (m.slot_bytes == 0) continue;
        if (m.slot_bytes < 0 || (m.slot_bytes & 15) || m.slot_offset < 0 || (m.slot_offset & 15) ||
            m.slot_offset > slots_bytes || m.slot_bytes > slots_bytes - m.slot_offset)
            return LLFE_ERR_INVALID;
    }
    return llfe::fan_out(n, threads, status, [&](int i) {
        const llfe_jpeg_image &m = images[i];
        memset(&descs[i], 0, sizeof descs[i]);  // n_comp 0: nothing staged for this image
        return m.slot_bytes == 0 ? LLFE_ERR_UNSUPPORTED
               : !data[i]        ? LLFE_ERR_INVALID
               : m.height <= 0 || m.width <= 0 || m.height > 65535 || m.width > 65535
                   ? LLFE_ERR_CAPACITY  // (no JPEG has that size)
                   : llfe_jpeg::read_coefs(data[i], (size_t)sizes[i], m.height, m.width, slots + m.slot_offset,
                                           m.slot_bytes, &descs[i], (flags & LLFE_JPEG_ORIENT) != 0);
    });
}

extern "C" int llfe_jpeg_parse_batch_flags(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height,
                                           int32_t width, uint8_t *staging, int64_t record_stride, int64_t slot_stride,
                                           llfe_jpeg_desc *descs, llfe_jpeg_scan *scans, int32_t *status, int32_t threads,
                                           uint32_t flags) {
    if ((flags & ~LLFE_JPEG_PARSE_RESTARTS) || n < 0 || (n && (!data || !sizes || !staging || !descs || !scans || !status)) || height <= 0 || width <= 0 ||
        height > 65535 || width > 65535 || slot_stride < 0 || record_stride < LLFE_JPEG_RECORD_HEADER ||
        (record_stride & 15))
        return LLFE_ERR_INVALID;
    return llfe::fan_out(n, threads, status, [&](int i) {
        memset(&descs[i], 0, sizeof descs[i]);  // n_comp 0, blocks_in_mcu 0: nothing staged for this image
        memset(&scans[i], 0, sizeof scans[i]);
        const int64_t off = (int64_t)i * record_stride;
        return data[i] ? llfe_jpeg::parse_one(data[i], (size_t)sizes[i], height, width, staging + off, off,
                                              record_stride, slot_stride, &descs[i], &scans[i],
                                              (flags & LLFE_JPEG_PARSE_RESTARTS) != 0)
                       : LLFE_ERR_INVALID;
    });
}

extern "C" int llfe_jpeg_parse_batch(const uint8_t *const *data, const uint64_t *sizes, int32_t n, int32_t height,
                                     int32_t width, uint8_t *staging, int64_t record_stride, int64_t slot_stride,
                                     llfe_jpeg_desc *descs, llfe_jpeg_scan *scans, int32_t *status, int32_t threads) {
    return llfe_jpeg_parse_batch_flags(data, sizes, n, height, width, staging, record_stride, slot_stride, descs, scans,
                                       status, threads, 0);
}

namespace llfe_jpeg {
// the twin's loop over validated records; slot_of(i): where image i's slot starts
template <class SlotOf>
int reference_all(const uint8_t *staging, const llfe_jpeg_scan *scans, const llfe_jpeg_desc *descs, int n, int32_t *status,
                  bool one_piece, SlotOf slot_of) {
    try {
        for (int i = 0; i < n; i++)
            status[i] = scans[i].blocks_in_mcu == 0
                            ? LLFE_ERR_UNSUPPORTED
                            : (scans[i].restart_interval ? reference_one<true> : reference_one<false>)(
                                  staging + scans[i].record_offset, scans[i], descs[i], slot_of(i), one_piece);
    } catch (const std::bad_alloc &) {
        return LLFE_ERR_OOM;
    }
    return LLFE_OK;
}
}  // namespace llfe_jpeg

extern "C" int llfe_jpeg_entropy_reference(const uint8_t *staging, int64_t staging_bytes, const llfe_jpeg_scan *scans,
                                           const llfe_jpeg_desc *descs, int32_t n, int32_t h, int32_t w, uint8_t *slots,
                                           int64_t slot_stride, int32_t *status, int32_t one_piece) {
    if (n < 0 || (n && (!staging || !scans || !descs || !slots || !status)) || h <= 0 || w <= 0 || h > 65535 ||
        w > 65535 || slot_stride <= 0 || staging_bytes < 0 || ((uintptr_t)staging & 15))
        return LLFE_ERR_INVALID;
    int max_sub = 0, max_blocks = 0;
    if (!llfe::check_jpeg_descs(descs, n, h, w, slot_stride) ||
        !llfe_huff::validate_scans(scans, descs, n, staging_bytes, &max_sub, &max_blocks))
        return LLFE_ERR_INVALID;
    return llfe_jpeg::reference_all(staging, scans, descs, n, status, one_piece != 0,
                                    [&](int i) { return slots + (size_t)i * (size_t)slot_stride; });
}

extern "C" int llfe_jpeg_entropy_reference_images(const uint8_t *staging, int64_t staging_bytes,
                                                  const llfe_jpeg_scan *scans, const llfe_jpeg_desc *descs,
                                                  const llfe_jpeg_image *images, int32_t n, uint8_t *slots,
                                                  int64_t slots_bytes, int32_t *status, int32_t one_piece) {
    if (n < 0 || (n && (!staging || !scans || !descs || !images || !slots || !status)) || slots_bytes < 0 ||
        staging_bytes < 0 || ((uintptr_t)staging & 15))
        return LLFE_ERR_INVALID;
    try {
        if (!llfe_huff::validate_scans_images(scans, descs, images, n, staging_bytes, slots_bytes)) return LLFE_ERR_INVALID;
    } catch (const std::bad_alloc &) {
        return LLFE_ERR_OOM;
    }
    return llfe_jpeg::reference_all(staging, scans, descs, n, status, one_piece != 0,
                                    [&](int i) { return slots + images[i].slot_offset; });
}

extern "C" int llfe_jpeg_records_layout(const uint64_t *sizes, const llfe_jpeg_image *images, int32_t n,
                                        int64_t *record_offsets, int64_t *staging_bytes) {
    if (n < 0 || !staging_bytes || (n && (!sizes || !images || !record_offsets))) return LLFE_ERR_INVALID;
    int64_t total = 0;
    for (int i = 0; i < n; i++) {
        record_offsets[i] = total;
        if (images[i].slot_bytes != 0) total += llfe_jpeg::record_bytes(sizes[i]);
    }
    *staging_bytes = total;
    return LLFE_OK;
}

extern "C" int llfe_jpeg_parse_images(const uint8_t *const *data, const uint64_t *sizes, int32_t n,
                                      const llfe_jpeg_image *images, const int64_t *record_offsets, uint8_t *staging,
                                      int64_t staging_bytes, llfe_jpeg_desc *descs, llfe_jpeg_scan *scans, int32_t *status,
                                      int32_t threads, uint32_t flags) {
    if ((flags & ~(LLFE_JPEG_PARSE_RESTARTS | LLFE_JPEG_ORIENT)) || n < 0 ||
        (n && (!data || !sizes || !images || !record_offsets || !staging || !descs || !scans || !status)) ||
        staging_bytes < 0)
        return LLFE_ERR_INVALID;
    for (int i = 0; i < n; i++) {  // every record inside the buffer, before the first byte is written
        if (images[i].slot_bytes == 0) continue;
        const int64_t off = record_offsets[i];
        if (sizes[i] >= ((uint64_t)1 << 40) || off < 0 || (off & 15) || off > staging_bytes ||
            llfe_jpeg::record_bytes(sizes[i]) > staging_bytes - off)
            return LLFE_ERR_INVALID;
    }
    return llfe::fan_out(n, threads, status, [&](int i) {
        const llfe_jpeg_image &m = images[i];
        memset(&descs[i], 0, sizeof descs[i]);  // n_comp 0, blocks_in_mcu 0: nothing staged for this image
        memset(&scans[i], 0, sizeof scans[i]);
        return m.slot_bytes == 0 ? LLFE_ERR_UNSUPPORTED
               : !data[i]        ? LLFE_ERR_INVALID
               : m.height <= 0 || m.width <= 0 || m.height > 65535 || m.width > 65535
                   ? LLFE_ERR_CAPACITY  // (no JPEG has that size)
                   : llfe_jpeg::parse_one(data[i], (size_t)sizes[i], m.height, m.width, staging + record_offsets[i],
                                          record_offsets[i], llfe_jpeg::record_bytes(sizes[i]), m.slot_bytes, &descs[i],
                                          &scans[i], (flags & LLFE_JPEG_PARSE_RESTARTS) != 0,
                                          (flags & LLFE_JPEG_ORIENT) != 0);
    });
}
