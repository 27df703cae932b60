// The entropy half of a baseline JPEG decode, written once for the device kernels
// (jpeg_huff.hip) and for their host twin (llfe_jpeg_entropy_reference, jpeg_decode.cpp): the
// bit reader, the decode tables and the decoding of one subsequence of the scan.
//
// Positions.  The scan's bytes are staged raw, stuffed FF 00 pairs included.  A position is
// raw byte * 8 + bit (bit 0 = the byte's most significant), always canonical: the byte is
// never the 00 of a stuffed pair.  Crossing a data byte advances the raw byte by one, by two
// when the byte was FF -- in marker-free entropy data every FF is followed by its stuffed 00
// (the parser refuses anything else), so the data bytes themselves say where the stuffing is.
//
// State.  (position, block within the MCU, coefficient index 0..63; 0 = the DC symbol is
// next).  A subsequence is decoded from an entry state until the position reaches its end
// byte; the exit state is the first symbol boundary at or past it.
//
// Restart intervals (records with restart_interval != 0; everything below marked RST, chosen
// per image, so a scan without them runs the code it always ran).  The scan then also holds
// markers FF D0..D7, byte-aligned, each behind an MCU boundary and 0..7 padding 1-bits, and the
// decoder state behind one is known: block 0 of the MCU, DC next.  A position never lies
// inside a marker.  The reader stops loading at a marker's FF (an FF followed by anything but
// 00) and hands out zero bits from there, and its byte accounting stops at that FF, so no bit
// of a marker or behind it is ever decoded as data.  A lane that stands in front of a marker
// at a symbol boundary crosses it at once, also when it has already reached its end byte: the
// position becomes the byte behind the marker and the state (0, 0), so a state is never on the
// near side of a marker it could cross.  Crossing at an MCU boundary with only 1-bits left in
// the byte is the regular case; a lane that gets there any other way (mid-block, or having
// consumed bits past the data) crosses all the same, so that its exit state is the true one
// whatever its entry state was, and its Marks say so (bad).
//
// Every read is bounded by the scan's staged length (bytes past it read as zero) and every
// table index is masked, so a wrong entry state or a corrupt stream decodes to garbage or to
// an anomaly, never to an access outside the record.
#ifndef LLFE_JPEG_HUFF_CORE_H
#define LLFE_JPEG_HUFF_CORE_H
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "jpeg_desc_check.h"
#include "llfe.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LLFE_HD __host__ __device__ __forceinline__
#else
#define LLFE_HD inline
#endif

namespace llfe_huff {

constexpr int kSub = 128;  // bytes of the scan per subsequence (one lane each)

// One Huffman table as the decoder reads it.  For a code length l, lim[l] is the first value
// of the next 16 bits of the stream that is not a code of length <= l (codes are canonical,
// so lim is monotone); the code of length l then is those 16 bits >> (16 - l), and its symbol
// vals[(off[l] + code) & 255].  lim[16] = 65536 for a complete code; values at or above
// lim[16] are no code at all.
struct Tab {
    uint32_t lim[18];
    int32_t off[18];
    uint8_t vals[256];
};
static_assert(sizeof(Tab) == LLFE_JPEG_HUFF_TABLE_BYTES, "decode table layout");

struct State {
    uint32_t pos;  // raw byte * 8 + bit; kNone: no state (an anomaly was met)
    uint32_t bz;   // block within the MCU << 8 | coefficient index
};
constexpr uint32_t kNone = 0xffffffffu;
LLFE_HD bool same(const State &a, const State &b) { return a.pos == b.pos && a.bz == b.bz; }

struct Reader {
    const uint8_t *d;
    int len;       // staged scan bytes
    uint64_t acc;  // data bytes (stuffing removed), the current one on top
    int nbytes;    // valid data bytes in acc
    int bo;        // bits of the top byte already consumed, 0..7
    int rb;        // raw index of the top byte
    int rp;        // raw index of the next byte to load
    bool ff;       // the last byte loaded was FF: a 00 that follows is stuffing
    int mk;        // RST: raw index of the FF of the marker the loads stopped at, kNoMark: none in sight
    bool over;     // RST: bits past the last data byte in front of that marker were consumed
};
constexpr int kNoMark = 0x7fffffff;

LLFE_HD void rd_init(Reader &r, const uint8_t *d, int len, uint32_t pos) {
    r.d = d;
    r.len = len;
    r.acc = 0;
    r.nbytes = 0;
    r.bo = (int)(pos & 7);
    r.rb = (int)(pos >> 3);
    r.rp = r.rb;
    r.ff = false;
    r.mk = kNoMark;
    r.over = false;
}

// top up to eight data bytes (at most sixteen raw bytes: one stuffed 00 per FF).  RST: up to
// the next marker, zeros from there
template <bool RST>
LLFE_HD void rd_fill(Reader &r) {
    for (int guard = 0; guard < 16 && r.nbytes < 8; guard++) {
        unsigned b = 0;
        if (RST) {
            if (r.rp >= 0 && r.rp < r.len && r.rp < r.mk) {
                b = r.d[r.rp];
                if (b != 0xff) {
                    r.rp++;
                } else if (r.rp + 1 < r.len && r.d[r.rp + 1] != 0) {
                    r.mk = r.rp;
                    b = 0;
                } else {
                    r.rp += 2;
                }
            }
        } else if (r.rp >= 0 && r.rp < r.len) {
            b = r.d[r.rp++];
            if (r.ff && b == 0) {
                r.ff = false;
                continue;
            }
            r.ff = b == 0xff;
        }
        r.acc |= (uint64_t)b << (56 - 8 * r.nbytes);
        r.nbytes++;
    }
}

// the k bits (1..32) that start `skip` bits after the current position; skip + k <= 57
LLFE_HD uint32_t rd_peek(const Reader &r, int skip, int k) { return (uint32_t)((r.acc << (r.bo + skip)) >> (64 - k)); }

// RST: the raw index stops at the marker in sight (the bytes from there are the reader's zeros,
// not the file's)
template <bool RST>
LLFE_HD void rd_skip(Reader &r, int n) {
    r.bo += n;
    while (r.bo >= 8 && r.nbytes > 0 && (!RST || r.rb < r.mk)) {
        r.rb += 1 + ((r.acc >> 56) == 0xff ? 1 : 0);
        r.acc <<= 8;
        r.nbytes--;
        r.bo -= 8;
    }
    if (RST && r.rb >= r.mk && r.bo > 0) {
        r.over = true;
        r.bo = 0;
    }
}

// the first position of subsequence i: its boundary byte, or the next one when the boundary
// falls on the 00 of a stuffed pair.  RST: a boundary on either byte of a marker starts behind
// the marker (where the lane in front of it ends up as well, having crossed it), and the guessed
// state (0, 0) is then the true one
template <bool RST>
LLFE_HD uint32_t sub_start(const uint8_t *d, int len, int i) {
    int b = i * kSub;
    if (RST) {
        if (b > 0 && b < len && d[b - 1] == 0xff) b++;
        else if (b + 1 < len && d[b] == 0xff && d[b + 1] != 0) b += 2;
    } else if (b > 0 && b < len && d[b] == 0 && d[b - 1] == 0xff) {
        b++;
    }
    if (b > len) b = len;
    return (uint32_t)b * 8u;
}

// where block `blk` (scan order) lives: its component, and its coefficients in the slot, or
// nullptr for the padding blocks of an edge MCU
struct Geometry {
    const llfe_jpeg_scan *sc;
    const llfe_jpeg_desc *d;
    uint8_t *slot;
};
LLFE_HD int16_t *locate(const Geometry &g, int blk, int *comp) {
    const llfe_jpeg_scan &sc = *g.sc;
    const int mcu = blk / sc.blocks_in_mcu, bi = blk - mcu * sc.blocks_in_mcu;
    const int my = mcu / sc.mcus_w, mx = mcu - my * sc.mcus_w;
    const int c = sc.blk_comp[bi & 7] % 3;
    *comp = c;
    const int col = mx * sc.comp_hs[c] + sc.blk_x[bi & 7], row = my * sc.comp_vs[c] + sc.blk_y[bi & 7];
    if (col >= g.d->comp[c].blocks_w || row >= g.d->comp[c].blocks_h) return nullptr;
    return (int16_t *)(g.slot + g.d->comp[c].coef_offset + ((int64_t)row * g.d->comp[c].blocks_w + col) * 128);
}

// RST: what one decode_sub saw of restart markers, for the verification.  `bad`: a marker was
// crossed other than at an MCU boundary behind 0..7 one-bits, is not FF D0..D7, or two markers
// crossed by this one decode are not restart_interval MCUs apart with consecutive indices.
struct Marks {
    int32_t n;      // markers crossed
    int32_t first;  // blocks completed in front of the first of them
    int32_t idx;    // its index (Dn - D0)
    int32_t bad;
};

// Decode from `in` until the position reaches byte `end` (<= len) or, with WRITE, block
// `total` is reached.  *blocks counts the blocks completed.  With WRITE the coefficients go
// to the slot in natural order (`nat`: zigzag index -> natural index) and every block's DC
// difference, padding blocks included, to dcd[block]; `first` is the index of the block the
// entry state is in.  Trailing 1-padding inside the scan's last byte ends the scan: the exit
// position is then len * 8.  An anomaly (no such code, a coefficient index past 63, a DC
// category above 11, an AC category above 10) returns pos = kNone.  RST: markers are crossed
// as described at the top, *marks (may be null) says what was seen; a crossing advances two raw
// bytes and takes one iteration, so the iteration bound holds.
template <bool WRITE, bool RST>
LLFE_HD State decode_sub(const uint8_t *scan, int len, const Tab *tabs, const llfe_jpeg_scan &sc, State in, int end,
                         int *blocks, const uint8_t *nat, const Geometry &g, int16_t *dcd, int first, int total,
                         Marks *marks) {
    Reader r;
    rd_init(r, scan, len, in.pos);
    int b = (int)(in.bz >> 8) & 7, z = (int)(in.bz & 63);
    const int bim = sc.blocks_in_mcu;
    if (b >= bim) b = 0;
    int done = 0, blk = first, comp = 0;
    int16_t *dst = nullptr;
    if (WRITE && blk < total) dst = locate(g, blk, &comp);
    Marks m{0, 0, 0, 0};
    int m_done = 0, m_idx = 0;  // of the last marker crossed
    if (RST && marks) *marks = m;
    const int cap = (end - r.rb) * 8 + 16;  // a symbol is at least one bit
    for (int it = 0; it < cap && (RST || (r.rb < end && (!WRITE || blk < total))); it++) {
        rd_fill<RST>(r);
        if (RST) {
            if (r.mk != kNoMark) {  // a marker is in sight: does the position stand in front of it?
                const unsigned top = (unsigned)(r.acc >> 56), rest = 0xffu >> r.bo;
                if (r.rb == r.mk || (r.bo > 0 && r.rb + 1 + (top == 0xff ? 1 : 0) == r.mk && (top & rest) == rest)) {
                    const int idx = (int)scan[r.mk + 1] - 0xd0;  // (mk + 1 < len: rd_fill looked at it)
                    if (b != 0 || z != 0 || r.over || idx < 0 || idx > 7) m.bad = 1;
                    if (m.n == 0) {
                        m.first = done;
                        m.idx = idx & 7;
                    } else if (done - m_done != sc.restart_interval * bim || (idx & 7) != ((m_idx + 1) & 7)) {
                        m.bad = 1;
                    }
                    m_done = done;
                    m_idx = idx & 7;
                    m.n++;
                    rd_init(r, scan, len, (uint32_t)(r.mk + 2) * 8u);
                    b = z = 0;
                    continue;
                }
            }
            if (!(r.rb < end && (!WRITE || blk < total))) break;
        }
        if (r.bo > 0 && r.rb >= len - 2) {  // only 1-padding left in the last data byte?
            const unsigned top = (unsigned)(r.acc >> 56), rest = 0xffu >> r.bo;
            if (r.rb + 1 + (top == 0xff ? 1 : 0) == len && (top & rest) == rest) {
                r.rb = len;
                r.bo = 0;
                break;
            }
        }
        const Tab &t = tabs[z == 0 ? (sc.blk_dc[b] & 1) : 2 + (sc.blk_ac[b] & 1)];
        const uint32_t p16 = rd_peek(r, 0, 16);
        int l = 1;
        while (l <= 16 && p16 >= t.lim[l]) l++;
        if (l > 16) return State{kNone, 0};
        const int sym = t.vals[(t.off[l] + (int)(p16 >> (16 - l))) & 255];
        const int s = sym & 15;
        int v = 0;
        if (s) {
            const int bits = (int)rd_peek(r, l, s);
            v = bits < (1 << (s - 1)) ? bits - (1 << s) + 1 : bits;
        }
        rd_skip<RST>(r, l + s);
        if (z == 0) {
            if (sym > 11) return State{kNone, 0};
            if (WRITE) dcd[blk] = (int16_t)v;
            z = 1;
        } else if (s == 0) {
            if ((sym >> 4) == 15) {
                z += 16;  // ZRL
                if (z > 64) return State{kNone, 0};
            } else {
                z = 64;  // EOB
            }
        } else {
            if (s > 10) return State{kNone, 0};
            z += sym >> 4;
            if (z > 63) return State{kNone, 0};
            if (WRITE && dst) dst[nat[z]] = (int16_t)v;
            z++;
        }
        if (z >= 64) {
            z = 0;
            b = b + 1 == bim ? 0 : b + 1;
            done++;
            blk++;
            if (WRITE && blk < total) dst = locate(g, blk, &comp);
        }
    }
    *blocks = done;
    if (RST && marks) *marks = m;
    return State{(uint32_t)r.rb * 8u + (uint32_t)r.bo, (uint32_t)b << 8 | (uint32_t)z};
}

// zigzag index -> natural (row-major) index
#define LLFE_JPEG_NATURAL_ORDER                                                                                      \
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, \
        28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,   \
        61, 54, 47, 55, 62, 63

LLFE_HD int subsequences(int scan_bytes) { return (scan_bytes + kSub - 1) / kSub; }

// The host check in front of the kernels and of their twin: every extent a record names lies
// inside the staging buffer, every selector inside its table, the restart interval one a DRI
// can hold, the MCU grid covers the block grids of the (already validated) descriptors.  On success the largest subsequence count and
// block count (padding blocks included) of an image.
inline bool validate_scans(const llfe_jpeg_scan *scans, const llfe_jpeg_desc *descs, int n, int64_t staging_bytes,
                           int *max_sub, int *max_blocks) {
    int ms = 0, mb = 0;
    for (int i = 0; i < n; i++) {
        const llfe_jpeg_scan &s = scans[i];
        if (s.blocks_in_mcu == 0) continue;
        const llfe_jpeg_desc &d = descs[i];
        if (d.n_comp != 1 && d.n_comp != 3) return false;
        if (s.record_offset < 0 || (s.record_offset & 15) || s.record_offset > staging_bytes) return false;
        const int64_t avail = staging_bytes - s.record_offset;
        auto inside = [&](int32_t off, int64_t bytes) { return off >= 0 && !(off & 15) && off <= avail && bytes <= avail - off; };
        if (s.scan_bytes < 1 || s.scan_bytes >= (1 << 28)) return false;
        if (!inside(s.quant_offset, 128 * (int64_t)d.n_comp) || !inside(s.table_offset, 4 * (int64_t)sizeof(Tab)) ||
            !inside(s.scan_offset, (((int64_t)s.scan_bytes + 15) & ~(int64_t)15) + 16))
            return false;
        if (s.blocks_in_mcu < 1 || s.blocks_in_mcu > 6 || s.mcus_w < 1 || s.mcus_h < 1) return false;
        if (s.restart_interval < 0 || s.restart_interval > 65535) return false;
        const int64_t blocks = (int64_t)s.mcus_w * s.mcus_h * s.blocks_in_mcu;
        if (blocks >= (1 << 30)) return false;
        for (int c = 0; c < d.n_comp; c++) {
            if (s.comp_hs[c] < 1 || s.comp_hs[c] > 2 || s.comp_vs[c] < 1 || s.comp_vs[c] > 2) return false;
            if ((int64_t)s.mcus_w * s.comp_hs[c] < d.comp[c].blocks_w || (int64_t)s.mcus_h * s.comp_vs[c] < d.comp[c].blocks_h)
                return false;
        }
        for (int b = 0; b < s.blocks_in_mcu; b++) {
            const int c = s.blk_comp[b];
            if (c >= d.n_comp || s.blk_dc[b] > 1 || s.blk_ac[b] > 1 || s.blk_x[b] >= s.comp_hs[c] || s.blk_y[b] >= s.comp_vs[c])
                return false;
        }
        ms = ms > subsequences(s.scan_bytes) ? ms : subsequences(s.scan_bytes);
        mb = mb > (int)blocks ? mb : (int)blocks;
    }
    *max_sub = ms;
    *max_blocks = mb;
    return true;
}

// The same check for images that each have their own size and tight slot
// (llfe_jpeg_entropy_decode_images and its host twin): every staged image's (blocks_in_mcu != 0)
// descriptor against its own height x width and slot_bytes, its slot 16-byte aligned, inside
// slots_bytes and apart from every other staged image's, and validate_scans for the records.
inline bool validate_scans_images(const llfe_jpeg_scan *scans, const llfe_jpeg_desc *descs, const llfe_jpeg_image *images,
                                  int n, int64_t staging_bytes, int64_t slots_bytes) {
    std::vector<std::pair<int64_t, int64_t>> ranges;  // [begin, end) of every slot
    for (int i = 0; i < n; i++) {
        if (scans[i].blocks_in_mcu == 0) continue;
        const llfe_jpeg_image &m = images[i];
        int64_t blocks = 0;
        if (m.height <= 0 || m.width <= 0 || m.height > 65535 || m.width > 65535 || m.slot_offset < 0 ||
            (m.slot_offset & 15) || m.slot_bytes <= 0 || (m.slot_bytes & 15) || m.slot_offset > slots_bytes ||
            m.slot_bytes > slots_bytes - m.slot_offset ||
            !llfe::check_jpeg_desc(descs[i], m.height, m.width, m.slot_bytes, &blocks))
            return false;
        ranges.emplace_back(m.slot_offset, m.slot_offset + m.slot_bytes);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); k++)
        if (ranges[k].first < ranges[k - 1].second) return false;
    int max_sub = 0, max_blocks = 0;
    return validate_scans(scans, descs, n, staging_bytes, &max_sub, &max_blocks);
}

}  // namespace llfe_huff
#endif
