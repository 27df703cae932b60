// EXIF orientation (tag 0x0112, values 1..8) as a re-indexing of the coded raster: where a pixel
// of the coded h x w image S lies in the result O that Pillow's ImageOps.exif_transpose (and so
// decode_bgr) returns.  Shared by the host twin (llfe_jpeg_orient_reference, jpeg_decode.cpp), the
// host check of llfe_jpeg_reconstruct_images_oriented and the kernel (jpeg_images.hip).  Plain
// C++ on the host, compiled for the device too.
//
//   o   result   O[y][x] =
//   1   h x w    S[y][x]
//   2   h x w    S[y][w-1-x]
//   3   h x w    S[h-1-y][w-1-x]
//   4   h x w    S[h-1-y][x]
//   5   w x h    S[x][y]
//   6   w x h    S[h-1-x][y]
//   7   w x h    S[h-1-x][w-1-y]
//   8   w x h    S[x][w-1-y]
#ifndef LLFE_JPEG_ORIENT_H
#define LLFE_JPEG_ORIENT_H
#include <cstdint>

#include "jpeg_desc_check.h"

namespace llfe {

LLFE_DESC_HD bool jpeg_orient_valid(int o) { return o >= 1 && o <= 8; }
// the result has the coded image's rows as its columns
LLFE_DESC_HD bool jpeg_orient_transposed(int o) { return o >= 5; }
// the kernel instantiation that writes the orientation: 0 upright (1), 1 mirrored in place
// (2, 3, 4), 2 transposed (5 .. 8)
constexpr int kJpegOrientGroups = 3;
LLFE_DESC_HD int jpeg_orient_group(int o) { return o == 1 ? 0 : o <= 4 ? 1 : 2; }
// the coded image's columns / rows run backwards in the result
LLFE_DESC_HD bool jpeg_orient_mirror_x(int o) { return o == 2 || o == 3 || o == 7 || o == 8; }
LLFE_DESC_HD bool jpeg_orient_mirror_y(int o) { return o == 3 || o == 4 || o == 6 || o == 7; }

// the result's row length in pixels (its row count is the other one of h, w)
LLFE_DESC_HD int jpeg_orient_row(int o, int h, int w) { return jpeg_orient_transposed(o) ? h : w; }

// the table above, inverted: pixel (y, x) of the coded h x w image lies at (*yr, *xr) of the
// result.  o in 1..8, 0 <= y < h, 0 <= x < w; then 0 <= *yr < rows, 0 <= *xr < jpeg_orient_row.
LLFE_DESC_HD void jpeg_orient_map(int o, int h, int w, int y, int x, int *yr, int *xr) {
    const int ym = jpeg_orient_mirror_y(o) ? h - 1 - y : y;
    const int xm = jpeg_orient_mirror_x(o) ? w - 1 - x : x;
    *yr = jpeg_orient_transposed(o) ? xm : ym;
    *xr = jpeg_orient_transposed(o) ? ym : xm;
}

}  // namespace llfe
#endif
