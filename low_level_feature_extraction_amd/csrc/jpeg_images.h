// llfe_jpeg_reconstruct_images (jpeg_images.hip): the tile of a sampling class and the records
// the host builds for the kernel.  Plain C++ on the host, compiled for the device too.
#ifndef LLFE_JPEG_IMAGES_H
#define LLFE_JPEG_IMAGES_H
#include <cstdint>

#include "jpeg_desc_check.h"

namespace llfe {

// The output tile of one workgroup and its planes in LDS.  A tile starts at a multiple of the
// class's MCU (tw and th are multiples of 16).  Luma: tbw x tbh blocks.  Chroma: cbw x cbh
// blocks per component, which start hx block columns left of and hy block rows above the
// tile's own chroma blocks: fancy upsampling reads one sample beyond the tile's chroma region
// on each side (columns for h2v1 and h2v2, rows too for h2v2), so the neighbouring blocks that
// hold those samples are transformed as well.  Pitches: the smallest p >= the plane's width
// with p % 32 == 16, for which the eight-byte row stores of two blocks (16 lanes, rows p apart,
// blocks 8 apart) fall on 32 different banks.
struct JpegTiling {
    int tw, th;      // output pixels
    int tbw, tbh;    // luma blocks
    int cbw, cbh;    // chroma blocks per component, halo included (0 for grey)
    int hx, hy;      // halo blocks in front of the tile's own
    int ypitch, cpitch;
};
constexpr int kJpegImgYBytes = 144 * 64;  // the largest luma plane (4:2:0: 128 x 64 at pitch 144)
constexpr int kJpegImgCBytes = 80 * 48;   // the largest chroma plane (4:2:0: 80 x 48 at pitch 80)
// orientations 5 .. 8 stage a tile in result order, a dword per pixel, tw rows at a pitch of
// th + 3 dwords, in the kernel's IDCT scratch of [8][9]-int tiles: the largest is 4:2:0's
constexpr int kJpegOrientStageTiles = (128 * (64 + 3) + 71) / 72;

LLFE_DESC_HD bool jpeg_tiling(int sampling, JpegTiling *t) {
    switch (sampling) {
    case LLFE_JPEG_GRAY: *t = JpegTiling{128, 32, 16, 4, 0, 0, 0, 0, 144, 0}; return true;
    case LLFE_JPEG_444: *t = JpegTiling{64, 32, 8, 4, 8, 4, 0, 0, 80, 80}; return true;
    case LLFE_JPEG_422: *t = JpegTiling{128, 32, 16, 4, 10, 4, 1, 0, 144, 80}; return true;
    case LLFE_JPEG_420: *t = JpegTiling{128, 64, 16, 8, 10, 6, 1, 1, 144, 80}; return true;
    }
    return false;
}

// one image of the call: its validated descriptor and where its slot and its result lie
struct JpegImageRec {
    llfe_jpeg_desc d;
    int64_t slot_offset, out_offset;  // bytes from coefs / out
    int32_t h, w;
    int32_t tiles_x;  // tiles per row of tiles
    int32_t vec;      // the result's rows are 4-byte aligned: dword stores
    int32_t orient;   // EXIF orientation 1 .. 8 (jpeg_orient.h); h, w stay the coded size
};
struct JpegWork {
    int32_t image, tile;
};

}  // namespace llfe
#endif
