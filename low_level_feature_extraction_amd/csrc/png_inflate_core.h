// PNG decoding behind the chunk walk, written once for the device kernels (png_inflate.hip)
// and for their host twin (llfe_png_decode_reference, png_decode.cpp): the bit reader, the
// canonical Huffman tables, the deflate block decoder, the per-pixel unfilter and Adler-32.
//
// Input.  One record per image: the deflate stream (the concatenated IDAT payloads without the
// two zlib header bytes and the four Adler-32 bytes), 16-byte aligned and followed by at least
// 16 zero bytes.  The reader loads aligned dwords and never one that starts at or past the padded length; what lies past it reads as zero.
//
// Output.  The decoder does not store bytes itself: it hands literals, matches and stored runs
// to a Sink.  The host sink writes them into the raw buffer, which is also its window; the
// device sink (png_inflate.hip) keeps the window in an LDS ring and lets the whole wave copy.
// A Sink also says which of `lanes()` cooperating lanes the caller is (`lane()`), makes the
// tables one lane wrote visible to the others (`sync()`) and broadcasts a value all lanes hold
// alike (`uniform()`): on the host one lane, no-ops.  All lanes run the same control flow.
//
// Termination.  Every block consumes at least three bits and every symbol at least one, and
// both loops stop once more bits were consumed than the stream has; the code-length loop is
// bounded by 286 + 30 symbols and the table builds by 288.  Arbitrary bytes end in a status,
// never in a read or a write outside what the descriptor names.
//
// Any anomaly ends the image with a non-zero code (the kE* below); the caller hands the image
// back to the host decoders, which stay the judge of what a broken file means.
#ifndef LLFE_PNG_INFLATE_CORE_H
#define LLFE_PNG_INFLATE_CORE_H
#include <cstdint>
#include <cstring>

#include "llfe.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LLFE_PNG_HD __host__ __device__ __forceinline__
#else
#define LLFE_PNG_HD inline
#endif

namespace llfe_png {

constexpr int kFastBits = 10;          // codes up to this length decode in one lookup
constexpr uint32_t kWindow = 32768;    // the deflate window
constexpr uint32_t kAdlerMod = 65521;
constexpr int kLit = 288, kDist = 32;  // symbols of the fixed codes (286 / 287 and 30 / 31 never valid)

enum {
    kOk = 0,
    kEBlockType = 1,   // reserved block type 3
    kEStored = 2,      // LEN / NLEN mismatch
    kEInput = 3,       // input exhausted before the final block's end-of-block
    kEOutput = 4,      // output would pass raw_n
    kEShort = 5,       // final end-of-block before raw_n bytes
    kECode = 6,        // no such code
    kESymbol = 7,      // litlen 286 / 287, distance code 30 / 31
    kEDistance = 8,    // a distance beyond the bytes produced so far
    kEOver = 9,        // an over-subscribed set of code lengths
    kEIncomplete = 10, // an incomplete set other than the single-code case
    kEHeader = 11,     // a dynamic header zlib refuses (counts, a repeat without a length or past the end, no EOB code)
    kEFilter = 12,     // a filter byte above 4
    kEAdler = 13,
};

// One canonical code.  count[l] codes of length l; symbol[] the symbols in code order; fast[v]
// for the next kFastBits stream bits v: length << 9 | symbol of the code they start with, 0
// when that code is longer (or v starts none).
struct Huff {
    uint16_t count[16];
    uint16_t symbol[kLit];
    uint16_t fast[1 << kFastBits];
};

// the tables of one image (on the device: in LDS, shared by the wave)
struct Tables {
    Huff lit, dist;          // (dist also serves as the code-length code while a header is read)
    uint8_t lens[kLit + kDist];
    uint8_t cl[32];          // the 19 code-length code lengths
    int32_t rc;              // the building lane's verdict
};

// ---------------------------------------------------------------------------- the bit reader
struct Reader {
    const uint8_t *d;
    uint32_t len;     // stream bytes
    uint32_t padded;  // bytes that may be loaded: len rounded up to 16, plus 16
    uint32_t p;       // next byte to load, a multiple of 4
    uint64_t acc;     // the next bits, least significant first
    int nbits;
};

LLFE_PNG_HD uint32_t ld32(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(p);  // (records are 16-byte aligned, p a multiple of 4)
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}

LLFE_PNG_HD void rd_init(Reader &r, const uint8_t *d, uint32_t len) {
    r.d = d;
    r.len = len;
    r.padded = ((len + 15u) & ~15u) + 16u;
    r.p = 0;
    r.acc = 0;
    r.nbits = 0;
}
// at least 33 bits afterwards (zeros past the padded stream)
LLFE_PNG_HD void rd_fill(Reader &r) {
    if (r.nbits <= 32) {
        const uint32_t v = r.p < r.padded ? ld32(r.d + r.p) : 0u;
        r.acc |= (uint64_t)v << r.nbits;
        r.p += 4;
        r.nbits += 32;
    }
}
LLFE_PNG_HD uint32_t rd_bits(Reader &r, int n) {  // n <= 32, n <= nbits
    const uint32_t v = (uint32_t)(r.acc & (((uint64_t)1 << n) - 1));
    r.acc >>= n;
    r.nbits -= n;
    return v;
}
// more bits consumed than the stream has
LLFE_PNG_HD bool rd_over(const Reader &r) { return (int64_t)r.p * 8 - r.nbits > (int64_t)r.len * 8; }
// continue at byte `off` (<= len)
LLFE_PNG_HD void rd_seek(Reader &r, uint32_t off) {
    r.p = off & ~3u;
    r.acc = 0;
    r.nbits = 0;
    rd_fill(r);
    rd_bits(r, (int)(off & 3u) * 8);
}

// ---------------------------------------------------------------------------- tables
enum { kCodes = 0, kLens = 1, kDists = 2 };

// the code the bits v (least significant first) start with, among lengths 1..maxlen:
// length << 9 | symbol, or 0
LLFE_PNG_HD uint32_t walk(const Huff &h, uint32_t v, int maxlen) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= maxlen; l++) {
        code |= (int)(v & 1u);
        v >>= 1;
        const int cnt = h.count[l];
        if (code - cnt < first) return (uint32_t)l << 9 | h.symbol[index + (code - first)];
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
    }
    return 0;
}

// n <= 288 code lengths (0..15) -> h.  Lane 0 counts, checks and sorts; all lanes fill fast[].
template <class Sink>
LLFE_PNG_HD int build(Tables &T, Huff &h, const uint8_t *lens, int n, int kind, Sink &s) {
    s.sync();  // the lengths are written
    if (s.lane() == 0) {
        for (int l = 0; l < 16; l++) h.count[l] = 0;
        for (int i = 0; i < n; i++) h.count[lens[i] & 15]++;
        int left = 1, rc = kOk;
        for (int l = 1; l < 16; l++) {
            left = left * 2 - h.count[l];
            if (left < 0) {
                rc = kEOver;
                break;
            }
        }
        const int codes = n - h.count[0];
        // zlib's rule: an incomplete set only as a single code of length 1 (or, for distances,
        // no code at all: a block of literals), never for the code-length code
        if (rc == kOk && left > 0 &&
            !(kind != kCodes && ((codes == 1 && h.count[1] == 1) || (codes == 0 && kind == kDists))))
            rc = kEIncomplete;
        if (rc == kOk) {
            uint16_t *offs = h.fast;  // (scratch until the fill below)
            offs[1] = 0;
            for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
            for (int i = 0; i < n; i++)
                if (lens[i] & 15) h.symbol[offs[lens[i] & 15]++] = (uint16_t)i;
        }
        T.rc = rc;
    }
    s.sync();
    const int rc = (int)s.uniform((uint32_t)T.rc);
    if (rc != kOk) return rc;
    for (uint32_t v = (uint32_t)s.lane(); v < (1u << kFastBits); v += (uint32_t)s.lanes())
        h.fast[v] = (uint16_t)walk(h, v, kFastBits);
    s.sync();
    return kOk;
}

// the next symbol, not yet consumed: length << 9 | symbol, 0: no such code.  Wants 15 bits.
LLFE_PNG_HD uint32_t peek(const Huff &h, const Reader &r) {
    const uint32_t v = (uint32_t)r.acc;
    const uint32_t e = h.fast[v & ((1u << kFastBits) - 1)];
    return e ? e : walk(h, v, 15);
}

// ---------------------------------------------------------------------------- blocks
template <class Sink>
LLFE_PNG_HD int stored_block(Reader &r, Sink &s, uint32_t raw_n) {
    rd_bits(r, r.nbits & 7);
    rd_fill(r);
    const uint32_t v = s.uniform(rd_bits(r, 32));
    const uint32_t len = v & 0xffffu;
    if ((len ^ 0xffffu) != v >> 16) return kEStored;
    const uint32_t off = r.p - (uint32_t)(r.nbits >> 3);  // (nbits is a multiple of 8 here)
    if (off > r.len || len > r.len - off) return kEInput;
    if (len > raw_n - s.pos()) return kEOutput;
    s.stored(r.d + off, len);
    rd_seek(r, off + len);
    return kOk;
}

template <class Sink>
LLFE_PNG_HD int fixed_tables(Tables &T, Sink &s) {
    s.sync();  // (nobody still reads the previous block's lengths)
    for (int i = s.lane(); i < kLit + kDist; i += s.lanes())
        T.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    int rc = build(T, T.lit, T.lens, kLit, kLens, s);
    if (rc == kOk) rc = build(T, T.dist, T.lens + kLit, kDist, kDists, s);
    return rc;
}

template <class Sink>
LLFE_PNG_HD int dynamic_tables(Reader &r, Tables &T, Sink &s) {
    rd_fill(r);
    const uint32_t hd = s.uniform(rd_bits(r, 14));
    const int nlen = (int)(hd & 31) + 257, ndist = (int)(hd >> 5 & 31) + 1, ncode = (int)(hd >> 10) + 4;
    if (nlen > 286 || ndist > 30) return kEHeader;
    s.sync();
    for (int i = s.lane(); i < 32; i += s.lanes()) T.cl[i] = 0;
    s.sync();
    for (int i = 0; i < ncode; i++) {
        rd_fill(r);
        const uint32_t l = rd_bits(r, 3);
        // the order of the code-length code lengths, three bits each: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
        if (s.lane() == 0) T.cl[at] = (uint8_t)l;
    }
    if (rd_over(r)) return kEInput;
    int rc = build(T, T.dist, T.cl, 19, kCodes, s);
    if (rc != kOk) return rc;
    int i = 0, prev = -1;
    while (i < nlen + ndist) {  // every round stores at least one length
        rd_fill(r);
        const uint32_t e = s.uniform(peek(T.dist, r));
        if (!e) return kECode;
        rd_bits(r, (int)(e >> 9));
        const int sym = (int)(e & 511);
        int rep = 1, val = sym;
        if (sym == 16) {
            if (prev < 0) return kEHeader;
            val = prev;
            rep = 3 + (int)rd_bits(r, 2);
        } else if (sym == 17) {
            val = 0;
            rep = 3 + (int)rd_bits(r, 3);
        } else if (sym == 18) {
            val = 0;
            rep = 11 + (int)rd_bits(r, 7);
        }
        rep = (int)s.uniform((uint32_t)rep);
        if (rep > nlen + ndist - i) return kEHeader;
        if (s.lane() == 0)
            for (int k = 0; k < rep; k++) T.lens[i + k] = (uint8_t)val;
        i += rep;
        prev = val;
        if (rd_over(r)) return kEInput;
    }
    s.sync();
    if (s.uniform(T.lens[256]) == 0) return kEHeader;  // no end-of-block code
    // the distance lengths follow the literal lengths directly; the literal table is built from
    // the first nlen, so move nothing: build reads lens + nlen
    rc = build(T, T.lit, T.lens, nlen, kLens, s);
    if (rc == kOk) rc = build(T, T.dist, T.lens + nlen, ndist, kDists, s);
    return rc;
}

// the symbols of one fixed or dynamic block, up to its end-of-block
template <class Sink>
LLFE_PNG_HD int coded_block(Reader &r, Tables &T, Sink &s, uint32_t raw_n) {
    for (;;) {  // every round consumes at least one bit
        rd_fill(r);
        const uint32_t e = s.uniform(peek(T.lit, r));
        if (!e) return kECode;
        rd_bits(r, (int)(e >> 9));
        const uint32_t sym = e & 511;
        if (sym < 256) {
            if (s.pos() >= raw_n) return kEOutput;
            s.literal((uint8_t)sym);
        } else if (sym == 256) {
            return rd_over(r) ? kEInput : kOk;
        } else {
            const uint32_t ls = sym - 257;
            if (ls > 28) return kESymbol;
            const int lx = ls < 8 || ls == 28 ? 0 : (int)(ls - 4) >> 2;
            uint32_t len = ls < 8 ? 3 + ls : ls == 28 ? 258 : 3 + ((4 + (ls & 3)) << lx);
            len += rd_bits(r, lx);  // (at most 15 + 5 of the 33 bits so far)
            rd_fill(r);
            const uint32_t de = s.uniform(peek(T.dist, r));
            if (!de) return kECode;
            rd_bits(r, (int)(de >> 9));
            const uint32_t ds = de & 511;
            if (ds > 29) return kESymbol;
            const int dx = ds < 4 ? 0 : (int)(ds - 2) >> 1;
            uint32_t dist = ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << dx);
            dist += rd_bits(r, dx);  // (15 + 13 bits)
            len = s.uniform(len);
            dist = s.uniform(dist);
            if (dist > s.pos()) return kEDistance;
            if (len > raw_n - s.pos()) return kEOutput;
            s.match(dist, len);
        }
        if (rd_over(r)) return kEInput;
    }
}

// the whole stream: exactly raw_n bytes into the sink, or a code
template <class Sink>
LLFE_PNG_HD int inflate(Reader &r, Tables &T, Sink &s, uint32_t raw_n) {
    for (;;) {  // every block consumes at least three bits
        rd_fill(r);
        const uint32_t hd = s.uniform(rd_bits(r, 3));
        const uint32_t type = hd >> 1;
        int rc;
        if (type == 0) {
            rc = stored_block(r, s, raw_n);
        } else if (type == 3) {
            rc = kEBlockType;
        } else {
            rc = type == 1 ? fixed_tables(T, s) : dynamic_tables(r, T, s);
            if (rc == kOk) rc = coded_block(r, T, s, raw_n);
        }
        if (rc != kOk) return rc;
        if (rd_over(r)) return kEInput;
        if (hd & 1) break;
    }
    return s.pos() == raw_n ? kOk : kEShort;
}

// ---------------------------------------------------------------------------- the host sink
// (also what a single device thread would use: raw is the window)
struct FlatSink {
    uint8_t *raw;
    uint32_t n;
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() {}
    uint32_t uniform(uint32_t v) const { return v; }
    uint32_t pos() const { return n; }
    void literal(uint8_t b) { raw[n++] = b; }
    void match(uint32_t dist, uint32_t len) {
        for (uint32_t i = 0; i < len; i++, n++) raw[n] = raw[n - dist];
    }
    void stored(const uint8_t *src, uint32_t len) {
        memcpy(raw + n, src, len);
        n += len;
    }
};

// ---------------------------------------------------------------------------- Adler-32
// the recurrence: (a, b) over n more bytes; sums stay below 2^32 for 5552 bytes at a time
inline uint32_t adler32(const uint8_t *p, size_t n) {
    uint32_t a = 1, b = 0;
    while (n) {
        const size_t k = n < 5552 ? n : 5552;
        for (size_t i = 0; i < k; i++) {
            a += p[i];
            b += a;
        }
        a %= kAdlerMod;
        b %= kAdlerMod;
        p += k;
        n -= k;
    }
    return b << 16 | a;
}
// The same in closed form, for lanes that each see some of the bytes: with n bytes d[g] in all,
// a = 1 + sum d[g] and b = n + sum (n - g) d[g], both mod 65521.  One aligned dword at g
// (bytes d0..d3) adds s = d0 + d1 + d2 + d3 to a and (n - g) s - (d1 + 2 d2 + 3 d3) to b.
LLFE_PNG_HD void adler_dword(uint64_t &a, uint64_t &b, uint32_t v, uint32_t g, uint32_t n) {
    const uint32_t d0 = v & 255, d1 = v >> 8 & 255, d2 = v >> 16 & 255, d3 = v >> 24;
    const uint32_t sum = d0 + d1 + d2 + d3;
    a += sum;
    b += (uint64_t)(n - g) * sum - (d1 + 2 * d2 + 3 * d3);
}
LLFE_PNG_HD void adler_byte(uint64_t &a, uint64_t &b, uint32_t d, uint32_t g, uint32_t n) {
    a += d;
    b += (uint64_t)(n - g) * d;
}

// ---------------------------------------------------------------------------- unfilter
// One pixel of three channels packed in bits 0..23 (any channel order: the filters are per
// channel).  x: the filtered bytes, a / b / c: the left, upper and upper-left pixels (0 outside
// the image); f: the row's filter type 0..4, a select per type and no branch.
LLFE_PNG_HD uint32_t unfilter_px(int f, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t o = 0;
    for (int sh = 0; sh < 24; sh += 8) {
        const int xa = (int)(a >> sh & 255), xb = (int)(b >> sh & 255), xc = (int)(c >> sh & 255);
        const int p = xa + xb - xc;
        const int pa = p > xa ? p - xa : xa - p, pb = p > xb ? p - xb : xb - p, pc = p > xc ? p - xc : xc - p;
        const int paeth = (pa <= pb && pa <= pc) ? xa : (pb <= pc ? xb : xc);
        const int pred = f == 1 ? xa : f == 2 ? xb : f == 3 ? (xa + xb) >> 1 : f == 4 ? paeth : 0;
        o |= (uint32_t)(((int)(x >> sh & 255) + pred) & 255) << sh;
    }
    return o;
}

// ---------------------------------------------------------------------------- descriptors
// n descriptors against (h, w), the staging buffer and the raw stride: false for a record
// outside the buffer or a geometry that is not h x w at 3 or 4 bytes per pixel
inline bool validate_png_descs(const llfe_png_desc *descs, int n, int h, int w, int64_t staging_bytes,
                               int64_t raw_stride) {
    for (int i = 0; i < n; i++) {
        const llfe_png_desc &d = descs[i];
        if (d.deflate_bytes == 0) continue;
        if (d.deflate_bytes < 0 || d.deflate_bytes > 0x7fffffff - 64) return false;
        if (d.bpp != 3 && d.bpp != 4) return false;
        if ((int64_t)d.row_bytes != (int64_t)w * d.bpp) return false;
        if (d.raw_bytes != (int64_t)h * ((int64_t)d.row_bytes + 1) || d.raw_bytes > 0x7fffffff || d.raw_bytes > raw_stride)
            return false;
        const int64_t need = (((int64_t)d.deflate_bytes + 15) & ~(int64_t)15) + 16;
        if (d.record_offset < 0 || (d.record_offset & 15) || d.record_offset > staging_bytes ||
            need > staging_bytes - d.record_offset)
            return false;
    }
    return true;
}

}  // namespace llfe_png
#endif
