"""Shared by test_jpeg_hand_inputs.py (CPU) and test_gpu_jpeg_hand.py: baseline JPEG files written
by hand from the syntax of the standard, for the device entropy decode (csrc/jpeg_huff.hip, its
host twin llfe_jpeg_entropy_reference, the parser llfe_jpeg_parse_batch) and the reconstruction
kernels.  An encoder emits a small corner of what the syntax allows; these files reach the rest:
16-bit codes as the common case, every (run, size) symbol, end-of-block aliases, needless and
overflowing ZRLs, categories the tables hold but the device does not take, zero padding, table
selectors and DHT layouts of every kind, component ids, 16-bit quantisation tables, DC sums that
leave 16 bits, blocks longer than a subsequence, the densest scan there is, and restart markers
placed by hand.  `walk` decodes a scan symbol by symbol, so a test can show that the list covers
what it claims.

CASES: dicts of name, blob, h, w, kind, restarts.  kind "ok": parser, twin and device take the
file and the slots equal decode.stage_coefs; "handed_back": the parser takes it, twin and device
hand it back; "parse": the parser refuses it.  The pixels are decode.decode_bgr's in every case.
"""
import functools
import struct

import numpy as np

from low_level_feature_extraction_amd import _lib

SUB = _lib.JPEG_SUBSEQUENCE_BYTES
JFIF = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
GREY = [(1, 1, 1, 0)]  # components: (id, h, v, quantisation table)
S420 = [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
S422 = [(1, 2, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
S444 = [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]

DC_SYMS = list(range(12))
AC_SYMS = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]


def adobe(transform):
    return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])


# ------------------------------------------------------------------------------ Huffman tables
def skewed(symbols):
    """[(length, symbol)]: the first eight symbols get the lengths 1..8, all the rest length 16,
    so 16-bit codes are the common case and the all-ones code stays unused."""
    return [(k + 1 if k < 8 else 16, s) for k, s in enumerate(symbols)]


def canon(table):
    """[(length, symbol)] -> (the 16 counts, the symbols by length, {symbol: (code, length)}):
    the canonical code of the standard (Annex C): codes of one length are consecutive in the
    order listed, the first code of a length is twice the one behind the last of the length before."""
    counts, vals, codes, code = [0] * 16, [], {}, 0
    for l in range(1, 17):
        for n, s in table:
            if n == l:
                codes[s] = (code, l)
                vals.append(s)
                counts[l - 1] += 1
                code += 1
        code <<= 1
    assert len(vals) == len(table) and len(codes) == len(vals)
    return counts, vals, codes


SKEW_DC, SKEW_AC = skewed(DC_SYMS), skewed(AC_SYMS)
PLAIN = [[(0, 0, SKEW_DC)], [(1, 0, SKEW_AC)]]  # DHT segments of (class, id, table)
COLOUR = PLAIN + [[(0, 1, skewed(DC_SYMS[::-1]))], [(1, 1, skewed(AC_SYMS[::-1]))]]


# ------------------------------------------------------------------------------ the bit writer
class Bits:
    """MSB first; a data byte FF is followed by a stuffed 00."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc = self.acc << n | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            self.n -= 8
            b = self.acc >> self.n & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def pad(self, ones=True):
        k = -self.n % 8
        if k:
            self.put((1 << k) - 1 if ones else 0, k)
        return k


def tokens_of(blocks, pattern, sel, ri=0, rst=lambda k: k & 7, eob=0x00):
    """Coefficient blocks (64 integers in zigzag order, the DC as its true value, which may leave
    16 bits) in scan order -> tokens (class, table, symbol, extra bits, count), with the DC
    prediction per component, ZRL for runs above 15 and `eob` behind a block that ends early.
    ri: after every ri MCUs the predictors reset and the token ("rst", rst(k)) stands for the
    k-th marker (none where rst gives None)."""
    toks, pred = [], [0] * len(sel)
    for i, blk in enumerate(blocks):
        assert len(blk) == 64
        mcu, bi = divmod(i, len(pattern))
        if ri and bi == 0 and mcu and mcu % ri == 0:
            pred = [0] * len(sel)
            if rst(mcu // ri - 1) is not None:
                toks.append(("rst", rst(mcu // ri - 1)))
        c = pattern[bi]
        td, ta = sel[c]
        diff, pred[c] = int(blk[0]) - pred[c], int(blk[0])
        s = abs(diff).bit_length()
        toks.append((0, td, s, diff if diff >= 0 else diff + (1 << s) - 1, s))
        run, last = 0, max([z for z in range(1, 64) if blk[z]], default=0)
        for z in range(1, last + 1):
            v = int(blk[z])
            if v == 0:
                run += 1
                continue
            while run > 15:
                toks.append((1, ta, 0xF0, 0, 0))
                run -= 16
            s = abs(v).bit_length()
            toks.append((1, ta, run << 4 | s, v if v >= 0 else v + (1 << s) - 1, s))
            run = 0
        if last < 63:
            toks.append((1, ta, eob, 0, 0))
    return toks


def emit(tokens, codes, ones=True):
    """tokens -> (the entropy-coded bytes, the padding bits at the end).  A marker gets one-padding
    in front of it and no stuffing."""
    bw = Bits()
    for t in tokens:
        if t[0] == "rst":
            bw.pad()
            bw.out += bytes([0xFF, 0xD0 + t[1]])
        elif t[0] == "bits":  # bits that are no code of the table
            bw.put(t[1], t[2])
        else:
            cls, tid, sym, bits, n = t
            bw.put(*codes[cls, tid][sym])
            if n:
                bw.put(bits, n)
    k = bw.pad(ones)
    return bytes(bw.out), k


# ------------------------------------------------------------------------------ the file
def grid(h, w, comps):
    """(the component of every block of an MCU, the number of MCUs).  One component is not
    interleaved: a block per MCU whatever its sampling factors say."""
    if len(comps) == 1:
        return [0], -(-h // 8) * -(-w // 8)
    mh, mv = max(c[1] for c in comps), max(c[2] for c in comps)
    return [c for c, k in enumerate(comps) for _ in range(k[1] * k[2])], -(-h // (8 * mv)) * -(-w // (8 * mh))


def _seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def _dht(tables):
    body = b""
    for cls, tid, table in tables:
        counts, vals, _ = canon(table)
        body += bytes([cls << 4 | tid]) + bytes(counts) + bytes(vals)
    return _seg(0xC4, body)


def jpeg(h, w, comps=GREY, blocks=None, tokens=None, dht=PLAIN, sel=None, qts=None, lead=JFIF, dht_first=False, ri=None,
         rst=lambda k: k & 7, eob=0x00, ones=True, tail=b"", need_padding=False):
    """One baseline file.  qts: {table number: 64 entries (zigzag order), or (entries, True) for a
    16-bit DQT}; dht: DHT segments in file order, a later table of a class and id replaces an
    earlier one; sel: (DC, AC) table per component; the scan from `blocks` (tokens_of) or from
    raw `tokens`; ri: the DRI's value (None: no DRI); tail: bytes between the scan and the EOI."""
    sel = sel or [(0, 0)] + [(1, 1)] * (len(comps) - 1)
    qts = qts or {k[3]: [1] * 64 for k in comps}
    codes = {(cls, tid): canon(table)[2] for seg in dht for cls, tid, table in seg}
    pattern, n_mcu = grid(h, w, comps)
    if tokens is None:
        assert len(blocks) == n_mcu * len(pattern), (len(blocks), n_mcu, len(pattern))
        tokens = tokens_of(blocks, pattern, sel, ri or 0, rst, eob)
    scan, padding = emit(tokens, codes, ones)
    assert padding or not need_padding
    out = b"\xff\xd8" + lead
    dhts = b"".join(_dht(seg) for seg in dht)
    if dht_first:
        out += dhts
    for tq, q in sorted(qts.items()):
        q, wide = q if isinstance(q, tuple) else (q, False)
        out += _seg(0xDB, bytes([wide << 4 | tq]) + (b"".join(struct.pack(">H", v) for v in q) if wide else bytes(q)))
    out += _seg(0xC0, struct.pack(">BHHB", 8, h, w, len(comps)) + b"".join(bytes([k[0], k[1] << 4 | k[2], k[3]]) for k in comps))
    if not dht_first:
        out += dhts
    if ri is not None:
        out += _seg(0xDD, struct.pack(">H", ri))
    out += _seg(0xDA, bytes([len(comps)]) + b"".join(bytes([k[0], td << 4 | ta]) for k, (td, ta) in zip(comps, sel)) +
                b"\x00\x3f\x00")
    return out + scan + tail + b"\xff\xd9"


# ------------------------------------------------------------------------------ the walker
def walk(blob) -> dict:
    """Decode the scan of a hand-made (well-formed) file symbol by symbol, from the file's own
    segments: the AC symbols, DC categories and code lengths that occur, the blocks, the markers,
    the scan's bytes and the longest and shortest block in bytes."""
    b, p = bytes(blob), 2
    tabs, comps, sel, ri = {}, [], [], 0
    while True:
        assert b[p] == 0xFF
        m, ln = b[p + 1], struct.unpack(">H", b[p + 2:p + 4])[0]
        s = b[p + 4:p + 2 + ln]
        if m == 0xC4:
            q = 0
            while q < len(s):
                counts = s[q + 1:q + 17]
                vals, tab, code, k = s[q + 17:q + 17 + sum(counts)], {}, 0, 0
                for l in range(1, 17):
                    for _ in range(counts[l - 1]):
                        tab[l, code] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                tabs[s[q] >> 4, s[q] & 15] = tab
                q += 17 + len(vals)
        elif m == 0xC0:
            h, w = struct.unpack(">HH", s[1:5])
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])]
        elif m == 0xDD:
            ri = struct.unpack(">H", s)[0]
        elif m == 0xDA:
            sel = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(s[0])]
            break
        p += 2 + ln
    scan = b[p + 2 + ln:b.rindex(b"\xff\xd9")]
    pattern, n_mcu = grid(h, w, comps)
    r = {"ac": set(), "dc": set(), "lengths": set(), "blocks": 0, "markers": [], "scan_bytes": len(scan),
         "longest": 0.0, "shortest": float("inf")}
    pieces, q = [], 0  # the intervals between markers, unstuffed
    while True:
        k = q
        while True:
            k = scan.find(b"\xff", k)
            if k < 0 or scan[k + 1] != 0:
                break
            k += 2
        pieces.append(scan[q:k if k >= 0 else len(scan)].replace(b"\xff\x00", b"\xff"))
        if k < 0:
            break
        assert 0xD0 <= scan[k + 1] <= 0xD7
        r["markers"].append(scan[k + 1] - 0xD0)
        q = k + 2
    mcu = 0
    for piece in pieces:
        bits, pos = bin(int.from_bytes(b"\x01" + piece, "big"))[3:], 0

        def symbol(tab):
            nonlocal pos
            for l in range(1, 17):
                if (l, int(bits[pos:pos + l], 2)) in tab:
                    pos += l
                    r["lengths"].add(l)
                    return tab[l, int(bits[pos - l:pos], 2)]
            raise ValueError("no such code")

        for _ in range(min(ri or n_mcu, n_mcu - mcu)):
            for c in pattern:
                start, z = pos, 1
                cat = symbol(tabs[0, sel[c][0]])
                r["dc"].add(cat)
                pos += cat
                while z < 64:
                    s = symbol(tabs[1, sel[c][1]])
                    r["ac"].add(s)
                    if s & 15 == 0 and s != 0xF0:
                        break
                    z += (s >> 4) + 1
                    pos += s & 15
                assert z <= 64 and pos <= len(bits)
                r["blocks"] += 1
                r["longest"], r["shortest"] = max(r["longest"], (pos - start) / 8), min(r["shortest"], (pos - start) / 8)
            mcu += 1
        assert len(bits) - pos < 8 and "0" not in bits[pos:]
    assert mcu == n_mcu
    return r


# ------------------------------------------------------------------------------ contents
def _value(rng, s):
    v = int(rng.integers(1 << (s - 1), 1 << s))
    return v if rng.integers(2) else -v


def rand_block(rng, density, sizes, dc=0):
    """DC `dc`; every AC coefficient is non-zero with probability `density`, its size uniform
    over `sizes`."""
    blk = [dc] + [0] * 63
    for z in range(1, 64):
        if rng.random() < density:
            blk[z] = _value(rng, int(rng.choice(sizes)))
    return blk


def skew_blocks(n=12):
    """n random blocks, density 1.0 down to 0, sizes 1..10; the DC differences have the
    categories 0, 1, .. 11 (and again)."""
    rng, out, dc = np.random.default_rng(16), [], 0
    for k in range(n):
        c = k % 12
        dc += (-1) ** c * ((1 << c) - 1)
        out.append(rand_block(rng, 1.0 - k / (n - 1), range(1, 11), dc))
    return out


def extreme_blocks(n):
    """Every (run 0..15, size 1..10) once, the values going round -(2^s-1), -2^(s-1), 2^(s-1),
    2^s-1 per size; the DC alternates 1023 / -1024; coefficient 63 is set in every other block."""
    todo = [(r, s) for r in range(16) for s in range(1, 11)]
    turn, out = {s: 0 for s in range(1, 11)}, []

    def value(s):
        turn[s] += 1
        return (-(2 ** s - 1), -2 ** (s - 1), 2 ** (s - 1), 2 ** s - 1)[turn[s] % 4]

    while todo or len(out) < n:
        blk, z = [1023 if len(out) % 2 == 0 else -1024] + [0] * 63, 1
        for r, s in list(todo):
            if z + r <= 62:
                blk[z + r] = value(s)
                z += r + 1
                todo.remove((r, s))
        if len(out) % 2 == 1:
            blk[63] = value(1 + len(out) // 2 % 10)
        out.append(blk)
    assert len(out) == n, len(out)
    return out


def long_block_list(n):
    """n blocks of 63 coefficients of size 9..10: under the skewed tables every one is a 16-bit
    code and 9 or 10 bits, so a block is some 200 bytes."""
    rng = np.random.default_rng(64)
    return [rand_block(rng, 1.0, (9, 10), int(rng.integers(-500, 500))) for _ in range(n)]


def quant_blocks(rng=None):
    """Small coefficients (sizes 1..4) at density 1.0 and 0.1, a DC-only block and a block with
    one coefficient in row 1 (zigzag index 2): the whole-block DC shortcut beside the full pass."""
    rng = rng or np.random.default_rng(40)
    one = [3] + [0] * 63
    one[2] = -2
    return [rand_block(rng, 1.0, range(1, 5), 5), rand_block(rng, 0.1, range(1, 5), -7), [9] + [0] * 63, one]


def big_blocks(rng, n):
    return [rand_block(rng, (1.0, 0.3, 0.05)[k % 3], range(1, 11), int(rng.integers(-1000, 1001))) for k in range(n)]


def mixed_table(seed):
    return [int(v) for v in np.random.default_rng(seed).integers(1, 65536, 64)]


@functools.lru_cache(maxsize=None)
def long_blocks_3wg():
    """(blob, h, w): long_block_list at the smallest grey size, 128 wide, whose scan exceeds
    2 x 256 subsequences: three workgroups of lanes."""
    def blob(rows):
        return jpeg(8 * rows, 128, blocks=long_block_list(16 * rows))

    rows = 2 * 256 * SUB // walk_scan_bytes(blob(1)) - 1  # (an estimate to start from)
    assert walk_scan_bytes(blob(rows)) <= 2 * 256 * SUB
    while walk_scan_bytes(blob(rows)) <= 2 * 256 * SUB:
        rows += 1
    return blob(rows), 8 * rows, 128


def walk_dri(blob):
    """The value of the file's DRI segment, 0 without one."""
    p = bytes(blob).find(b"\xff\xdd\x00\x04")
    return 0 if p < 0 else struct.unpack(">H", blob[p + 4:p + 6])[0]


def walk_scan_bytes(blob):
    b = bytes(blob)
    sos = b.index(b"\xff\xda")
    return b.rindex(b"\xff\xd9") - (sos + 2 + (b[sos + 2] << 8 | b[sos + 3]))


@functools.lru_cache(maxsize=None)
def stuffed_before_marker():
    """Grey 8 x 96 with a marker behind every block, one of them behind a stuffed FF 00 pair."""
    for seed in range(400):
        rng = np.random.default_rng(5000 + seed)
        blob = jpeg(8, 96, blocks=[rand_block(rng, 0.5, range(1, 11), int(rng.integers(-200, 200))) for _ in range(12)], ri=1)
        scan = blob[-2 - walk_scan_bytes(blob):-2]
        if any(scan[k:k + 3] == b"\xff\x00\xff" and 0xD0 <= scan[k + 3] <= 0xD7 for k in range(len(scan) - 3)):
            return blob
    raise AssertionError("no stuffed pair in front of a marker")


# ------------------------------------------------------------------------------ the list
CASES = []


def add(name, h, w, kind="ok", restarts=False, **kw):
    blob = kw.pop("blob", None) or jpeg(h, w, **kw)
    CASES.append({"name": name, "h": h, "w": w, "blob": blob, "kind": kind, "restarts": restarts})


def _dc(v=0):
    return (0, 0, abs(v).bit_length(), v if v >= 0 else v + (1 << abs(v).bit_length()) - 1, abs(v).bit_length())


ZRL, EOB = (1, 0, 0xF0, 0, 0), (1, 0, 0x00, 0, 0)


def _build():
    rng = np.random.default_rng(2024)
    # ---- symbols, lengths and block ends
    add("skew16", 24, 32, blocks=skew_blocks())
    add("extremes", 40, 40, blocks=extreme_blocks(25))
    only = [0] * 62 + [-3]
    add("only_63", 16, 16, blocks=[[5] + only, [-9] + [0] * 63, [40] + [0] * 62 + [1023], [0] * 64])
    alias = skewed(AC_SYMS[:4] + [0x50] + AC_SYMS[4:])
    add("eob_alias", 16, 16, blocks=[rand_block(rng, d, range(1, 11), k) for k, d in enumerate((0.5, 0.1, 0.0, 0.9))],
        dht=[[(0, 0, SKEW_DC)], [(1, 0, alias)]], eob=0x50)
    add("zrl_then_eob", 8, 16, tokens=[_dc(3), ZRL, ZRL, ZRL, EOB, _dc(-2), (1, 0, 0x01, 1, 1), ZRL, ZRL, ZRL, EOB])
    # (beyond the three ZRLs above: one that lands exactly on index 64 and so ends the block itself)
    add("zrl_lands_on_64", 8, 16, tokens=[_dc(3), (1, 0, 0xE1, 0, 1), ZRL, ZRL, ZRL, _dc(-2), ZRL, ZRL, (1, 0, 0xE3, 5, 3), ZRL])
    add("zrl_x4", 8, 16, "handed_back", tokens=[_dc(3), ZRL, ZRL, ZRL, ZRL, _dc(-2), EOB])
    add("run_overflow", 8, 16, "handed_back", tokens=[_dc(3), ZRL, ZRL, ZRL, (1, 0, 0xF1, 1, 1), _dc(-2), EOB])
    add("dc_cat12", 8, 16, "handed_back", tokens=[(0, 0, 12, 0xABC, 12), EOB, _dc(1), EOB],
        dht=[[(0, 0, skewed(DC_SYMS + [12]))], [(1, 0, SKEW_AC)]])
    add("ac_size11", 8, 16, "handed_back", tokens=[_dc(3), (1, 0, 0x0B, 0x5A5, 11), EOB, _dc(1), EOB],
        dht=[[(0, 0, SKEW_DC)], [(1, 0, skewed(AC_SYMS + [0x0B]))]])
    # (FFFF is no code of a skewed table: behind it six bits and an EOB, so that a decoder which took it for the
    # 16-bit code next to the last one -- symbol 06 -- would find a well-formed scan)
    add("no_such_code", 8, 16, "handed_back", tokens=[_dc(3), ("bits", 0xFFFF, 16), ("bits", 0x20, 6), EOB, _dc(-2), EOB])
    # ---- the end of the scan
    few = [rand_block(rng, 0.3, range(1, 6), k) for k in range(4)]
    add("zero_padding", 16, 16, "handed_back", blocks=few, ones=False, need_padding=True)
    add("extra_byte", 16, 16, "handed_back", blocks=few, tail=b"\x7f")
    add("fill_ff", 16, 16, "parse", blocks=few, tail=b"\xff")
    add("all_ones_code", 16, 16, "parse", blocks=[[0] * 64] * 4, dht=[[(0, 0, [(1, 0), (1, 1)])], [(1, 0, SKEW_AC)]])
    # ---- the extremes of block length
    one_bit = [[(0, 0, [(1, 0)])], [(1, 0, [(1, 0x00)])]]
    add("densest", 512, 512, blocks=[[0] * 64] * 4096, dht=one_bit)
    add("long_blocks", 64, 64, blocks=long_block_list(64))
    blob, h, w = long_blocks_3wg()
    add("long_blocks_3wg", h, w, blob=blob)
    # ---- DC sums
    add("dc_wrap", 64, 64, blocks=[[2047 * (k + 1)] + [0] * 63 for k in range(64)])
    pattern, n_mcu = grid(265, 281, S420)
    seen = [0, 0, 0]
    wrap = []
    for k in range(n_mcu * 6):
        c = pattern[k % 6]
        seen[c] += 1
        wrap.append([2047 * seen[c]] + [0] * 63)
    add("dc_wrap_colour", 265, 281, comps=S420, dht=COLOUR, blocks=wrap)
    # ---- frames, selectors and DHT layouts
    add("grey_hv22", 16, 24, comps=[(1, 2, 2, 0)], blocks=big_blocks(rng, 6))
    add("grey_hv22_odd", 17, 25, comps=[(1, 2, 2, 0)], blocks=big_blocks(rng, 12))
    four = [[(0, 0, skewed(DC_SYMS[3:] + DC_SYMS[:3]))], [(1, 0, skewed(AC_SYMS[40:] + AC_SYMS[:40]))],
            [(0, 1, skewed(DC_SYMS[::-1]))], [(1, 1, skewed(AC_SYMS[::-1]))]]
    add("sel_swapped_420", 32, 32, comps=S420, dht=four, sel=[(1, 1), (0, 0), (0, 1)], blocks=big_blocks(rng, 24))
    add("sel_shared_444", 17, 9, comps=S444, sel=[(0, 0)] * 3, blocks=big_blocks(rng, 18))
    wrong = [(0, 0, skewed(DC_SYMS[::-1])), (1, 0, skewed(AC_SYMS[::-1]))]
    add("dht_layouts_one_segment", 24, 32, blocks=skew_blocks(), dht=[PLAIN[0] + PLAIN[1] + COLOUR[2] + COLOUR[3]])
    add("dht_layouts_redefined", 24, 32, blocks=skew_blocks(), dht=[wrong] + PLAIN)
    add("dht_layouts_before_sof", 24, 32, blocks=skew_blocks(), dht_first=True)
    add("ids_012", 16, 32, comps=[(0, 2, 1, 0), (1, 1, 1, 1), (2, 1, 1, 1)], dht=COLOUR, lead=b"", blocks=big_blocks(rng, 16))
    rgb = [(ord(c), 1, 1, 0) for c in "RGB"]
    add("ids_rgb", 16, 16, "parse", comps=rgb, dht=COLOUR, lead=b"", blocks=big_blocks(rng, 12))
    add("adobe_t0", 16, 16, "parse", comps=S444, dht=COLOUR, lead=adobe(0), blocks=big_blocks(rng, 12))
    add("adobe_t1", 16, 16, comps=S444, dht=COLOUR, lead=adobe(1), blocks=big_blocks(rng, 12))
    add("s440", 16, 16, "parse", comps=[(1, 1, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)], dht=COLOUR, blocks=big_blocks(rng, 8))
    add("s411", 16, 32, "parse", comps=[(1, 4, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)], dht=COLOUR, blocks=big_blocks(rng, 12))
    add("all_2x2", 16, 16, "parse", comps=[(1, 2, 2, 0), (2, 2, 2, 1), (3, 2, 2, 1)], dht=COLOUR, blocks=big_blocks(rng, 12))
    # ---- quantisation tables and reconstruction
    add("dqt16_ones", 16, 16, blocks=quant_blocks(), qts={0: ([1] * 64, True)})
    for v in (300, 1000, 40000, 65535):
        add(f"dqt16_{v}", 16, 16, blocks=quant_blocks(), qts={0: ([v] * 64, True)})
    add("dqt16_mixed", 16, 16, blocks=quant_blocks(), qts={0: (mixed_table(1), True)})
    add("q255_big", 16, 16, blocks=big_blocks(rng, 4), qts={0: [255] * 64})
    add("q1_big", 16, 16, blocks=big_blocks(rng, 4), qts={0: [1] * 64})
    for name, comps in (("colour_extremes_420", S420), ("colour_extremes_422", S422)):
        pattern, n_mcu = grid(17, 33, comps)
        blocks = [rand_block(rng, 0.2, range(1, 4), int(rng.integers(-8, 9))) if c == 0 else
                  rand_block(rng, 0.3, range(6, 11), int(rng.integers(-1000, 1001))) for _ in range(n_mcu) for c in pattern]
        add(name, 17, 33, comps=comps, dht=COLOUR, blocks=blocks, qts={0: (mixed_table(2), True), 1: (mixed_table(3), True)})
    # ---- restart intervals
    add("rst_ri1_skew", 8, 104, restarts=True, blocks=skew_blocks(13), ri=1)
    add("rst_after_stuffed", 8, 96, restarts=True, blob=stuffed_before_marker())
    add("rst_ri_larger_than_scan", 16, 16, restarts=True, blocks=few, ri=1000)
    # (five differences of 2047 stay inside 16 bits; with 20 to an interval every sum wraps again)
    for name, ri in (("rst_dc_wrap", 5), ("rst_dc_wrap_ri20", 20)):
        add(name, 64, 64, restarts=True, blocks=[[2047 * (k % ri + 1)] + [0] * 63 for k in range(64)], ri=ri)
    add("rst_long_blocks", 64, 64, restarts=True, blocks=long_block_list(64), ri=1)
    add("rst_wrong_index", 8, 96, "handed_back", restarts=True, blocks=skew_blocks(), ri=1, rst=lambda k: 2 * k & 7)
    add("rst_missing", 8, 96, "handed_back", restarts=True, blocks=skew_blocks(), ri=1,
        rst=lambda k: None if k == 4 else k & 7)


_build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RECON = [n for n in BY_NAME if n.startswith(("dqt16_", "q255", "q1_", "colour_extremes"))]


def by_size() -> dict:
    """(h, w, restarts) -> the cases of that size, in list order."""
    out = {}
    for c in CASES:
        out.setdefault((c["h"], c["w"], c["restarts"]), []).append(c)
    return out
