"""Hand-made PNG files for the device PNG decode (csrc/png_inflate_core.h, csrc/png_inflate.hip).

A PNG writer that lets a test choose what Pillow's does not: the filtered rows, the
zlib.compressobj (level, strategy, flushes), the IDAT split and the chunks around it; a bit
writer for deflate streams no encoder emits (every length and distance code, a code-length
repeat that crosses from the literal into the distance lengths, and the malformed ones); and a
small inflate walker that reports which codes a stream uses, so the case list can be shown to
cover them.  CASES is the list: dicts with name, blob, h, w and kind:
  "ok"       eligible and well formed: parse, twin and device status 0
  "parse"    handed back by the parse (status non-zero there)
  "anomaly"  staged, and refused by the twin and the device with a non-zero status
In every case the pixels are whatever decode.decode_batch makes of the file (or its error)."""
import struct
import zlib

import numpy as np

Z_RLE, Z_FIXED, Z_HUFFMAN_ONLY, Z_FILTERED = 3, 4, 2, 1
SIG = b"\x89PNG\r\n\x1a\n"


# ------------------------------------------------------------------------------ the writer
def chunk(typ: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def split_at(payload: bytes, cuts) -> list:
    """payload cut at the byte offsets `cuts` (repeated offsets give zero-length pieces)."""
    out, at = [], 0
    for c in list(cuts) + [len(payload)]:
        out.append(payload[at:c])
        at = c
    return out


def png(h, w, ctype, payload, pieces=None, depth=8, interlace=0, before=(), between=(), plte=None) -> bytes:
    """signature, IHDR, `before` chunks, [PLTE], the IDAT pieces (one IDAT with `payload` by
    default) with the `between` chunks behind the first piece, IEND."""
    out = [SIG, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))]
    out += list(before)
    if plte is not None:
        out.append(chunk(b"PLTE", plte))
    for k, p in enumerate(pieces if pieces is not None else [payload]):
        out.append(chunk(b"IDAT", p))
        if k == 0:
            out += list(between)
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(img, filters) -> bytes:
    """The filtered rows of img (h x w x c uint8, or h x rowbytes with bpp=...), row y with filter
    type filters[y % len(filters)]."""
    img = np.asarray(img, np.uint8)
    h = img.shape[0]
    bpp = img.shape[2] if img.ndim == 3 else 1
    rows = img.reshape(h, -1).astype(np.int32)
    n = rows.shape[1]
    out = bytearray()
    zero = np.zeros(n, np.int32)
    for y in range(h):
        f = filters[y % len(filters)]
        cur, up = rows[y], rows[y - 1] if y else zero
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        ul = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        if f == 0:
            pred = zero
        elif f == 1:
            pred = left
        elif f == 2:
            pred = up
        elif f == 3:
            pred = (left + up) >> 1
        else:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, ul)], np.int32)
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw: bytes, level=6, strategy=0, flush=None, stride=None, wbits=15, memlevel=8) -> bytes:
    """The zlib stream of raw; flush (zlib.Z_SYNC_FLUSH / Z_FULL_FLUSH) after every `stride` bytes."""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, memlevel, strategy)
    if flush is None:
        return co.compress(raw) + co.flush()
    out = b""
    for at in range(0, len(raw), stride):
        out += co.compress(raw[at:at + stride]) + co.flush(flush)
    return out + co.flush()


def idat_payload(blob: bytes) -> bytes:
    """The concatenated IDAT payloads of a PNG."""
    at, out = 8, b""
    while at + 12 <= len(blob):
        n, typ = struct.unpack(">I", blob[at:at + 4])[0], blob[at + 4:at + 8]
        if typ == b"IDAT":
            out += blob[at + 8:at + 8 + n]
        at += n + 12
    return out


# ------------------------------------------------------------------------------ deflate by hand
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canon(lens) -> dict:
    """symbol -> (code, length) of the canonical code with these lengths."""
    codes, code = {}, 0
    for ln in range(1, 16):
        for s, l_ in enumerate(lens):
            if l_ == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):  # n bits of v, least significant first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):  # a Huffman code (code, length): most significant bit first
        v, n = c
        for k in range(n - 1, -1, -1):
            self.put(v >> k & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self) -> bytes:
        self.align()
        return bytes(self.out)


def len_sym(n):
    s = max(k for k in range(29) if LBASE[k] <= n) if n < 258 else 28
    return s, n - LBASE[s]


def dist_sym(d):
    s = max(k for k in range(30) if DBASE[k] <= d)
    return s, d - DBASE[s]


def put_tokens(bw: Bits, tokens, lit, dist):
    """tokens: int literal | (length, distance) | ("lit", symbol) | ("dist", length, code, extra)."""
    for t in tokens:
        if isinstance(t, int):
            bw.code(lit[t])
        elif t[0] == "lit":  # a raw literal/length symbol (286, 287)
            bw.code(lit[t[1]])
        elif t[0] == "dist":  # a raw distance code (30, 31) behind a regular length
            s, x = len_sym(t[1])
            bw.code(lit[257 + s])
            bw.put(x, LEXT[s])
            bw.code(dist[t[2]])
            bw.put(t[3], 13)
        else:
            s, x = len_sym(t[0])
            bw.code(lit[257 + s])
            bw.put(x, LEXT[s])
            s, x = dist_sym(t[1])
            bw.code(dist[s])
            bw.put(x, DEXT[s])
    bw.code(lit[256])


def fixed_block(bw: Bits, tokens, final=True):
    bw.put(final, 1)
    bw.put(1, 2)
    put_tokens(bw, tokens, canon(FIXED_LIT), canon(FIXED_DIST))


def stored_block(bw: Bits, data: bytes, final=False, nlen=None):
    bw.put(final, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    bw.out += data


def dynamic_block(bw: Bits, lit_lens, dist_lens, cl_lens, cl_seq, tokens, final=True):
    """lit_lens / dist_lens: the full length lists (257.. / 1.. entries), cl_lens: the 19
    code-length code lengths, cl_seq: [(symbol, extra bits value)] that spells the two lists."""
    bw.put(final, 1)
    bw.put(2, 2)
    bw.put(len(lit_lens) - 257, 5)
    bw.put(len(dist_lens) - 1, 5)
    ncl = max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1
    ncl = max(ncl, 4)
    bw.put(ncl - 4, 4)
    for k in range(ncl):
        bw.put(cl_lens[CL_ORDER[k]], 3)
    cl = canon(cl_lens)
    for s, x in cl_seq:
        bw.code(cl[s])
        if s >= 16:
            bw.put(x, {16: 2, 17: 3, 18: 7}[s])
    put_tokens(bw, tokens, canon(lit_lens), canon(dist_lens))


def spell(lens):
    """(cl_lens, cl_seq) that spell a list of code lengths plainly: every length as itself, runs of
    zeros by 17 and 18, under one fixed complete code-length code (thirteen 4-bit, six 5-bit codes)."""
    seq, at = [], 0
    while at < len(lens):
        run = 0
        while at + run < len(lens) and lens[at + run] == 0 and run < 138:
            run += 1
        if run >= 11:
            seq.append((18, run - 11))
        elif run >= 3:
            seq.append((17, run - 3))
        else:
            run = 1
            seq.append((lens[at], 0))
        at += run
    return [4] * 13 + [5] * 6, seq


def replay(tokens, start=b"") -> bytes:
    """What the tokens inflate to (behind `start`)."""
    out = bytearray(start)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t[0], int):
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def zwrap(deflated: bytes, raw: bytes, adler=None) -> bytes:
    return b"\x78\x01" + deflated + struct.pack(">I", zlib.adler32(raw) if adler is None else adler)


# ------------------------------------------------------------------------------ the walker
def walk(stream: bytes) -> dict:
    """Inflate a deflate stream (no zlib header) symbol by symbol: the length codes, distance
    codes and code-length symbols it uses, its block types, the longest code length of a dynamic
    table and whether a code-length repeat crossed from the literal into the distance lengths."""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for k in range(n):
            v |= (stream[pos >> 3] >> (pos & 7) & 1) << k
            pos += 1
        return v

    def table(lens):
        return {(c, n): s for s, (c, n) in canon(lens).items()}

    def sym(tab):
        code = 0
        for n in range(1, 16):
            code = code << 1 | bits(1)
            if (code, n) in tab:
                return tab[(code, n)]
        raise ValueError("no such code")

    r = {"len": set(), "dist": set(), "cl": set(), "types": [], "maxlen": 0, "crossing": False, "out": 0}
    while True:
        final, typ = bits(1), bits(2)
        r["types"].append(typ)
        if typ == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            bits(16)
            pos += 8 * n
            r["out"] += n
        else:
            if typ == 1:
                lit, dist = table(FIXED_LIT), table(FIXED_DIST)
            else:
                nl, nd, nc = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for k in range(nc):
                    cl[CL_ORDER[k]] = bits(3)
                ct, lens = table(cl), []
                while len(lens) < nl + nd:
                    s = sym(ct)
                    r["cl"].add(s)
                    before = len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
                    if s >= 16 and before < nl < len(lens):
                        r["crossing"] = True
                r["maxlen"] = max(r["maxlen"], max(lens))
                lit, dist = table(lens[:nl]), table(lens[nl:])
            while True:
                s = sym(lit)
                if s == 256:
                    break
                if s < 256:
                    r["out"] += 1
                    continue
                r["len"].add(s)
                r["out"] += LBASE[s - 257] + bits(LEXT[s - 257])
                d = sym(dist)
                r["dist"].add(d)
                bits(DEXT[d])
        if final:
            return r


# ------------------------------------------------------------------------------ images
def noise(h, w, c=3, seed=0, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, c), dtype=np.uint8)


def smooth(h, w, c=3, seed=0):
    """A gradient with a little noise and flat bands: literals, short and long matches."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(3 * x + y) & 255, (x + 2 * y) & 255, (x * y) & 255, (x ^ y) & 255][:c], axis=2).astype(np.uint8)
    img[::3] = (img[::3] + rng.integers(0, 4, img[::3].shape)).astype(np.uint8)
    img[h // 3:h // 2] = 200
    return img


CASES = []
_CTYPE = {3: 2, 4: 6}


def add(name, h, w, blob, kind="ok", walked=False):
    CASES.append({"name": name, "h": h, "w": w, "blob": blob, "kind": kind, "walk": walked})


def add_img(name, img, filters=(0, 1, 2, 3, 4), pieces=None, kind="ok", walked=False, before=(), between=(), **z):
    h, w, c = img.shape
    payload = deflate(filter_rows(img, list(filters)), **z)
    add(name, h, w, png(h, w, _CTYPE[c], payload, pieces(payload) if pieces else None, before=before, between=between),
        kind, walked)


def _build():
    # ---- block types
    big = smooth(150, 150)  # raw 67650 bytes: more than one stored block
    add_img("stored_67650", big, level=0)
    blk = smooth(48, 64, seed=1)
    add_img("fixed", blk, strategy=Z_FIXED)
    add_img("level6", blk, level=6)
    add_img("level9", blk, level=9)
    add_img("level1", blk, level=1)
    add_img("huffman_only", blk, strategy=Z_HUFFMAN_ONLY)
    add_img("rle", blk, strategy=Z_RLE)
    add_img("filtered", blk, strategy=Z_FILTERED)
    stride = 64 * 3 + 1
    add_img("sync_flush_rows", blk, flush=zlib.Z_SYNC_FLUSH, stride=stride)
    add_img("full_flush_rows", blk, flush=zlib.Z_FULL_FLUSH, stride=stride)
    add_img("sync_flush_odd", blk, flush=zlib.Z_SYNC_FLUSH, stride=77)
    add_img("fixed_sync_flush", blk, strategy=Z_FIXED, flush=zlib.Z_SYNC_FLUSH, stride=50)
    add_img("wbits9", blk, level=9, wbits=9)
    # ---- matches
    flat = np.full((32, 300, 3), 77, np.uint8)
    add_img("flat_rows", flat, filters=(0,), level=9)
    add_img("flat_rgba_up", np.full((32, 300, 4), 9, np.uint8), filters=(2,), level=9)
    # rows of 4096 raw bytes, rows 8..15 repeat rows 0..7: the period is exactly 32768 (zlib itself
    # stops 262 short of its window; "all_codes" below holds a match at 32768 made by hand)
    far = noise(16, 1365, seed=2, hi=16)
    far[8:] = far[:8]
    add_img("period_32768", far, filters=(0,), level=9)
    farther = noise(16, 1366, seed=3, hi=16)
    farther[8:] = farther[:8]  # 32792: out of the window, no match
    add_img("period_32792", farther, filters=(0,), level=9)
    # every length code and every distance code, in one fixed block behind a stored one
    rng = np.random.default_rng(4)
    w_all = 100
    head = rng.integers(0, 5, 32800, dtype=np.uint8).tobytes()  # (bytes 0..4: any of them is a filter type)
    tokens = []
    for k in range(30):
        tokens.append((LBASE[k % 29] + (1 if LEXT[k % 29] else 0), DBASE[k] + ((1 << DEXT[k]) - 1)))
        tokens += [int(v) for v in rng.integers(0, 5, 3)]
    tokens.append((LBASE[28], 1))
    tokens.append((LBASE[27] + 30, 24577))
    body = replay(tokens, head)
    pad = -len(body) % (3 * w_all + 1)
    tokens += [int(v) for v in rng.integers(0, 5, pad)]
    body = replay(tokens, head)
    bw = Bits()
    stored_block(bw, head)
    fixed_block(bw, tokens)
    h_all = len(body) // (3 * w_all + 1)
    add("all_codes", h_all, w_all, png(h_all, w_all, 2, zwrap(bw.bytes(), body)), walked=True)
    # ---- code lengths
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(f, 10 + 7 * k, np.uint8) for k, f in enumerate(fib)])
    vals = np.concatenate([vals, np.full(100 * 96 * 3 - len(vals), 10 + 7 * 20, np.uint8)])  # (28656 -> 28800)
    vals = np.random.default_rng(5).permutation(vals)
    add_img("fibonacci", vals.reshape(100, 96, 3), filters=(0,), strategy=Z_HUFFMAN_ONLY, memlevel=9, walked=True)
    # whatever the zlib at hand makes of that, by hand: code lengths 1..15 for fifteen byte values and 15
    # for the end of block, a single distance code (the incomplete set zlib accepts), literals only
    values = [0] + [10 + 7 * k for k in range(14)]
    lit_lens = [0] * 257
    for k, v in enumerate(values):
        lit_lens[v] = k + 1
    lit_lens[256] = 15
    tk = []
    for y in range(8):
        tk += [0] + [values[(y * 24 + x) % 15] for x in range(24)]
    bw = Bits()
    dynamic_block(bw, lit_lens, [1], *spell(lit_lens + [1]), tk)
    add("lengths_1_to_15", 8, 8, png(8, 8, 2, zwrap(bw.bytes(), replay(tk))), walked=True)
    add_img("sparse_lengths", noise(40, 40, seed=6, lo=100, hi=103), filters=(0,), level=9, walked=True)
    # a code-length repeat that starts in the literal lengths and ends in the distance lengths:
    # lengths 2 for symbols 0, 255, 256, 257 and distance codes 0..3, spelled 2, 18 x 2, 2, 16 (x 6)
    lit_lens = [2] + [0] * 254 + [2, 2, 2]
    dist_lens = [2, 2, 2, 2]
    cl_lens = [0] * 19
    cl_lens[2], cl_lens[16], cl_lens[18] = 1, 2, 2
    cl_seq = [(2, 0), (18, 138 - 11), (18, 116 - 11), (2, 0), (16, 3)]
    hc, wc = 6, 5
    tk = []
    for y in range(hc):
        tk += [0, 255, 255, 0, (3, 1), 255, (3, 4), 255, (3, 2), 0]  # 16 bytes a row, the first a 0
    bw = Bits()
    dynamic_block(bw, lit_lens, dist_lens, cl_lens, cl_seq, tk)
    add("repeat_crossing", hc, wc, png(hc, wc, 2, zwrap(bw.bytes(), replay(tk))), walked=True)
    # ---- chunks
    img = smooth(40, 60, seed=7)
    add_img("idat_1_byte_each", img, pieces=lambda p: split_at(p, range(1, 301)))
    add_img("idat_empty_first_last_between", img, pieces=lambda p: split_at(p, [0, 0, 2, 2, 7, 100, 100, len(p) - 4, len(p), len(p)]))
    add_img("idat_split_in_header_and_adler", img, pieces=lambda p: split_at(p, [1, 3, len(p) - 5, len(p) - 2]))
    add_img("idat_split_7", img, pieces=lambda p: split_at(p, range(7, len(p), 7)))
    text = chunk(b"tEXt", b"Comment\0hand made")
    add_img("ancillary_before_and_between", img, pieces=lambda p: split_at(p, [len(p) // 2]),
            before=[text, chunk(b"gAMA", struct.pack(">I", 45455))], between=[text])
    # ---- filters
    for c in (3, 4):
        for f in range(5):
            add_img(f"filter{f}_c{c}", noise(9, 7, c, seed=10 + f), filters=(f,))
        pairs = [f for a in range(5) for b in range(5) for f in (a, b)]
        add_img(f"filter_pairs_c{c}", noise(50, 11, c, seed=20), filters=pairs)
        add_img(f"paeth_ties_c{c}", noise(20, 33, c, seed=21, lo=0, hi=3), filters=(4, 4, 3))
        add_img(f"saturated_c{c}", noise(20, 33, c, seed=22, lo=0, hi=2) * 255, filters=(4, 3, 4, 1, 3))
        add_img(f"carries_c{c}", noise(20, 33, c, seed=23, lo=250, hi=256), filters=(3, 4))
    # ---- sizes
    add_img("1x1", noise(1, 1, seed=30), filters=(4,))
    add_img("1x1_rgba", noise(1, 1, 4, seed=30), filters=(3,))
    add_img("1x37", noise(1, 37, seed=31), filters=(4,))
    add_img("37x1", noise(37, 1, seed=32))
    for h in (63, 64, 65, 129):
        add_img(f"h{h}", noise(h, 5, seed=33 + h), filters=(4, 3, 1, 2, 0, 4, 4))
        add_img(f"h{h}_rgba", noise(h, 3, 4, seed=33 + h), filters=(3, 4))
    for w in (1, 2, 4, 63, 64, 65, 257):
        add_img(f"w{w}", noise(3, w, seed=40 + w), filters=(1, 4, 3))
    add_img("w66_h70_rgba", smooth(70, 66, 4, seed=41), filters=(4, 3, 2, 1))
    # ---- handed back by the parse
    g = noise(10, 12, 1, seed=50)
    add("grey", 10, 12, png(10, 12, 0, deflate(filter_rows(g, [0, 1]))), "parse")
    add("grey_alpha", 10, 12, png(10, 12, 4, deflate(filter_rows(noise(10, 12, 2, seed=51), [4]))), "parse")
    add("palette", 10, 12, png(10, 12, 3, deflate(filter_rows(g % 7, [0])), plte=noise(1, 7, 3, seed=52).tobytes()), "parse")
    deep = noise(10, 12, 6, seed=53)
    add("rgb16", 10, 12, png(10, 12, 2, deflate(filter_rows(deep, [0, 2])), depth=16), "parse")
    im = noise(10, 12, seed=54)
    a7 = b""
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = im[y0::dy, x0::dx]
        if sub.size:
            a7 += filter_rows(sub, [0])
    add("interlaced", 10, 12, png(10, 12, 2, deflate(a7), interlace=1), "parse")
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(smooth(10, 12, seed=55)).save(buf, "JPEG", quality=90)
    add("jpeg", 10, 12, buf.getvalue(), "parse")
    add("other_size", 10, 12, png(11, 12, 2, deflate(filter_rows(noise(11, 12, seed=56), [1]))), "parse")
    add_img("good_10x12", noise(10, 12, seed=57))
    # ---- anomalies (10 x 12 RGB: 370 raw bytes)
    ah, aw = 10, 12
    aimg = smooth(ah, aw, seed=60)
    raw = filter_rows(aimg, [0, 1, 2, 3, 4])

    def anomaly(name, payload):
        add(name, ah, aw, png(ah, aw, 2, payload), "anomaly")

    for name, z in (("flip_level6", deflate(raw)), ("flip_stored", deflate(raw, level=0)), ("flip_fixed", deflate(raw, strategy=Z_FIXED))):
        # (a block type bit, the middle, the last byte but one of the deflate data: never a padding bit)
        for at in (2 * 8 + 1, len(z) * 4 + 1, (len(z) - 6) * 8 + 2):
            bad = bytearray(z)
            bad[at >> 3] ^= 1 << (at & 7)
            anomaly(f"{name}_bit{at}", bytes(bad))
    good = deflate(raw)
    anomaly("wrong_adler", good[:-4] + struct.pack(">I", zlib.adler32(raw) ^ 0x10000))
    rows = deflate(raw, flush=zlib.Z_SYNC_FLUSH, stride=37)
    anomaly("cut_before_final_block", rows[:len(rows) * 2 // 3])
    anomaly("cut_one_byte", good[:-5] + good[-4:])
    anomaly("final_block_early", deflate(raw[:185]))
    anomaly("one_byte_too_many", deflate(raw + b"\0"))
    for v in (5, 255):
        bad = bytearray(raw)
        bad[37 * 4] = v
        anomaly(f"filter_byte_{v}", deflate(bytes(bad)))
    small = [int(v) for v in np.random.default_rng(61).integers(0, 5, 370)]

    def hand(name, build, out=None):
        bw = Bits()
        build(bw)
        anomaly(name, zwrap(bw.bytes(), bytes(small) if out is None else out))

    hand("distance_before_start", lambda b: fixed_block(b, small[:2] + [(5, 3)] + small[7:]))
    hand("length_symbol_286", lambda b: fixed_block(b, small[:100] + [("lit", 286)] + small[100:]))
    hand("distance_code_30", lambda b: fixed_block(b, small[:100] + [("dist", 3, 30, 0)] + small[103:]))
    hand("block_type_3", lambda b: (stored_block(b, bytes(small[:100])), b.put(1, 1), b.put(3, 2), b.put(0, 32)))
    hand("stored_bad_nlen", lambda b: stored_block(b, bytes(small), final=True, nlen=0x1234))
    over = [0] * 19
    over[0], over[1], over[2] = 1, 1, 1
    hand("oversubscribed_code_lengths", lambda b: dynamic_block(b, [8] * 257, [5], over, [], []))
    incomplete = [0] * 19
    incomplete[0], incomplete[8] = 2, 2
    hand("incomplete_code_lengths", lambda b: dynamic_block(b, [8] * 257, [5], incomplete, [], []))
    hand("stored_longer_than_stream", lambda b: (b.put(1, 1), b.put(0, 2), b.align(), b.put(370, 16), b.put(370 ^ 0xffff, 16),
                                                 b.out.extend(bytes(small[:200]))))


_build()


def by_size() -> dict:
    """(h, w) -> the cases of that size, in list order."""
    out = {}
    for c in CASES:
        out.setdefault((c["h"], c["w"]), []).append(c)
    return out
