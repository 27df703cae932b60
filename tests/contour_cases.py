"""Masks for the GPU contour path (csrc/contours_gpu.hip) aimed at branches that random masks
and the workload's own images do not reach.

tests/test_contour_case_inputs.py checks on the CPU (host library, oracle, 8-connected
labelling) that every case is what its row says; tests/test_gpu_contour_cases.py runs the
same cases through ``find_contours_gpu``, ``shapes_from_masks_gpu`` and
``font_detect(binary=)``.  Both import the catalogue below, so a case cannot be edited in one
file only.  Masks are built once per case (``functools.lru_cache``): callers must not modify
them.

Words used below.  A *ring* is a closed 1-px rectangle outline, a *dot* an isolated pixel, a
*bar* two pixels one above the other.  The raster scan rejects a component when the last live
border mark it passed on the row (lnbd) is not a right-bound one.  A ring's left wall is visited
but never right-bound (its east neighbour is a hole, which the outer border never sweeps), so
whatever starts on a row behind it is rejected until an accepted border's right edge is passed.
Only a hole does that: the mouth of a C is swept from inside and its wall ends right-bound.  A
rejected component is never followed by OpenCV, so its pixels stay unmarked, while the device
has followed every component beforehand and must mask those marks.  On the row of a rejected
first pixel the scan resumes behind it with the lnbd it had, so such marks only count on the
rows below: a dot 3 px behind the *second* row of a rejected bar is rejected too, and is
accepted as soon as the bar's right-bound marks count as live.

  case                      shape      rejected  target
  A1 rej_grid               40x140     462       s_rej full (kRejBoxes = 64): ``hit`` forced, every run looked up.
                                                 154 triples (bar, dot behind its second row, dot behind its first row)
                                                 on rows 3 .. 34; a block east of the ring, first row 21, after the
                                                 65th rejection (row 6)
  A1 rej_64 / 65 / 66       40x140     64 65 66  64 of the triples: every box used; + a bar: the first component without
                                                 a box; + the dot behind its second row
  A1 rej_straddle_few       40x140     7         rejected blocks at x = 61..66, 62..65 and a 2x2 blob at 63..64, two rows
                                                 each, a dot 3 px behind the second row: the box test and the run walk
                                                 across a word edge
  A1 rej_straddle_many      40x140     77        the same behind 70 other rejections
  A2 wide_rej_W             15xW       >= 5      W = 4095, 4096: a ring 3900 .. W - 6, bars and their dots at x >= 4032
                                                 and over 4031 | 4032 (bar at 4030 / 4031, dot at 4033 / 4034): live
                                                 masking in the second 63-word window and its lane-0 word.  W = 4033: a
                                                 hole needs a wall to its right, so nothing can be rejected at x = 4032;
                                                 the ring closes at 4032 and the bars sit in and over word 62
  A3 far_W                  31xW       5 (1)     queries (dots) at x >= 4032 on rows with no foreground in 3968 .. x - 1:
                                                 (d) empty row: frame, start; (a) an accepted block's right edge: start;
                                                 (b) a dot rejected inside a ring, then the query: lnbd is still the
                                                 ring's wall, no start; (c) the wall alone: no start; (e) an accepted
                                                 dash ending at 3967 / at 3968, query at 4032: start; a ring's wall at
                                                 3967 / 3968: no start.  A mark left of 3968 is looked up in global
                                                 memory (pix_is_right_mark), one at 3968 in the window's lane-0 word.
                                                 W = 4033 has the rows that start only (no hole reaches x = 4032)
  A4 restarts               27x140     8         per row: accepted dot, dot rejected in a ring, accepted dot (lnbd is
                                                 that ring's right wall), dot rejected in a ring; inside one word
                                                 (x = 2 .. 23) and over 63 | 64 at three phases: bpos, seg, accm cut
  B5 corners(3, 4) / (4, 3) 64x128     0         all 4096 patterns of rows 30 .. and columns 62 .. over the tile corner
                            x 4096               (64, 32): links over the corner and over both edges next to it; a
                                                 12 x (12 + i % 7) block in tile (0, 0) so that every image keeps one
                                                 shape and k_ct_bases carries 1024, 2048, 3072 shapes
  B6 serpentine_S           S          0         first pixel in the last tile column, rows joined at alternate ends
  B6 corner_{ne,nw,se,sw}_S S          0         one component through a diagonal-only link over the corner (64, 32);
                                                 ne / nw: the raster-first pixel is a lone pixel of another tile
                                                 (S = 33x65, 64x128, 70x130: partial tiles)
  B7 spiral, diagonal,      200x300    0         1-px curves that leave the 64-row x 256-px LDS window of the tracer
     staircase, window_edge                      again and again, each with a 12x12 ring so that contourArea >= 100;
                                                 window_edge zigzags over y = 63 | 64 and x = 255 | 256
  B8 comb_{a..e}            see COMBS  0         one border of 1024, 1026, 8192, 8194 and 13 104 vertices: k_ct_shapes
                                                 from LDS / from global memory (kPtsLds = 1024), k_ct_trace staged /
                                                 followed a second time (kCtStage = 8192)
  B9 regrow                 399x1010   0         15 combs of 5862 vertices: 87 930 > 81 920 = 1 * 16384 + 65536

No entry documents a limit that a case exceeds (all are at most 4096 wide), so every case runs
through all three entries.
"""
from __future__ import annotations

import functools

import numpy as np

TW, TH = 64, 32          # labelling tile
REJ_BOXES = 64           # kRejBoxes
PTS_LDS = 1024           # kPtsLds
STAGE = 8192             # kCtStage
PTS_DEFAULT_1 = 16384 + 65536  # contours_default_caps(1).pts
WIN0 = 63 * 64           # first pixel of the second scan window (4032)
LANE0 = 62 * 64          # first pixel of the second window's lane-0 word (3968)
WIDE = (4033, 4095, 4096)
SIZES = ((33, 65), (64, 128), (70, 130))


def _ring(m, y0, x0, y1, x1, right=True):
    m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = 255
    m[y0:y1 + 1, x0] = 255
    if right:
        m[y0:y1 + 1, x1] = 255


# ------------------------------------------------------------------ A1
def _rej_mask(n, extra=None):
    """40x140: a ring (1,1)-(38,120) holding n components in triples -- a bar of two rows, a dot
    3 px behind the bar's second row, a dot 5 px behind its first row -- then ``extra`` (drawn
    inside the ring below them), and a block east of the ring on rows 21 .. 30.

    Marks of a rejected component matter on the rows below its first one (on that row the scan
    resumes behind it with the lnbd it had), hence the bars: the dot behind a bar's second row
    is accepted as soon as the bar's right-bound marks count as live."""
    m = np.zeros((40, 140), np.uint8)
    _ring(m, 1, 1, 38, 120)
    k = 0
    for y in range(3, 34, 3):
        for x in range(4, 112, 8):
            for ys, xx in ((slice(y, y + 2), x), (y + 1, x + 3), (y, x + 5)):
                if k < n:
                    m[ys, xx] = 255
                    k += 1
    assert k == n
    m[21:31, 125:136] = 255
    if extra is not None:
        extra(m)
    return m


def _straddles(m):
    m[27:29, 61:67] = 255
    m[28, 69] = 255       # block 61..66, a dot behind its second row
    m[27, 71] = 255       # ... and one on its first row
    m[30:32, 62:66] = 255
    m[31, 68] = 255       # block 62..65, dot
    m[33:35, 63:65] = 255
    m[34, 67] = 255       # 2x2 blob at 63..64, dot


def _bar_past_the_boxes(m):
    m[12:14, 20] = 255    # the 65th rejected component: no box is kept for it


def _bar_and_dot_past_the_boxes(m):
    _bar_past_the_boxes(m)
    m[13, 23] = 255       # the 66th: behind the second row of the 65th


@functools.lru_cache(maxsize=None)
def rej_grid():
    # 11 groups x 14 triples = 462 components on rows 3 .. 34; the 65th rejection is on row 6
    return _rej_mask(462)


@functools.lru_cache(maxsize=None)
def rej_n(n):
    # 64 of the triples (rows 3 .. 7), then one bar, then the dot behind it
    return _rej_mask(64, {64: None, 65: _bar_past_the_boxes, 66: _bar_and_dot_past_the_boxes}[n])


@functools.lru_cache(maxsize=None)
def rej_straddle(many):
    return _rej_mask(70 if many else 0, _straddles)


# ------------------------------------------------------------------ A2
def _closed(w):
    """A hole needs a wall to its right, so no first pixel of the last column can be rejected:
    at W = 4033 the second window (x = 4032 alone) can hold the wall only."""
    return w - 6 > WIN0 + 8   # room for queries at x = 4040 .. inside a ring that ends at W - 6


@functools.lru_cache(maxsize=None)
def wide_rej(w):
    """A ring from x = 3900 holding bars of two rows (x, first row) with a dot 3 px behind the
    second row, as in A1, and one pair of dots on a row."""
    m = np.zeros((15, w), np.uint8)
    if _closed(w):
        _ring(m, 1, 3900, 13, w - 6)
        bars = ((4040, 3), (4060, 3), (4030, 6), (4050, 6), (4031, 9), (4070, 9))
        m[11, [4036, 4039]] = 255          # a pair of dots on one row
    else:
        _ring(m, 1, 3900, 13, w - 1)
        bars = ((4027, 3), (3965, 6), (4020, 9))
        m[11, [3965, 3968]] = 255
    for x, y in bars:
        m[y:y + 2, x] = 255
        m[y + 1, x + 3] = 255
    return m


# ------------------------------------------------------------------ A3
def far_rows(w):
    """row -> (query x, starts a border, last foreground x left of the query or None)"""
    qx = 4050 if _closed(w) else WIN0
    rows = {
        1: (qx, True, None),            # (d)
        4: (qx, True, 3910),            # (a)
        15: (WIN0, True, LANE0 - 1),    # (e) accepted dash ending at 3967
        17: (WIN0, True, LANE0),        # (e) ... at 3968
    }
    if _closed(w):
        rows.update({
            9: (qx, False, 3900),           # (b)
            11: (qx, False, 3800),          # (c)
            21: (WIN0, False, LANE0 - 1),   # (e) wall at 3967
            27: (WIN0, False, LANE0),       # (e) wall at 3968
        })
    return rows


@functools.lru_cache(maxsize=None)
def far(w):
    m = np.zeros((31, w), np.uint8)
    xr = w - 2 if _closed(w) else w - 1
    m[3:6, 3900:3911] = 255             # (a) block
    _ring(m, 7, 3800, 13, xr)           # (b), (c)
    m[9, 3900] = 255                    # (b) the rejected dot
    m[15, 3960:LANE0] = 255             # (e) dashes
    m[17, 3960:LANE0 + 1] = 255
    _ring(m, 19, LANE0 - 1, 23, xr)     # (e) walls
    _ring(m, 25, LANE0, 29, xr)
    for y, (qx, _, _) in far_rows(w).items():
        m[y, qx] = 255
    return m


# ------------------------------------------------------------------ A4
RESTART_PHASES = (0, 44, 48, 54)


def restart_row_pixels(k):
    """(row, x of the accepted, rejected, accepted, rejected first pixels) of phase k"""
    y, o = 4 + 6 * k, RESTART_PHASES[k]
    return y, (2 + o, 8 + o, 14 + o, 20 + o)


@functools.lru_cache(maxsize=None)
def restarts():
    m = np.zeros((27, 140), np.uint8)
    for k, o in enumerate(RESTART_PHASES):
        y, xs = restart_row_pixels(k)
        m[y, list(xs)] = 255
        _ring(m, y - 2, 5 + o, y + 2, 11 + o)
        _ring(m, y - 2, 17 + o, y + 2, 23 + o)
    return m


# ------------------------------------------------------------------ B5
CORNER_X, CORNER_Y = 64, 32


@functools.lru_cache(maxsize=None)
def corners(ph, pw):
    """Every ph x pw bit pattern over the tile corner of a 64x128 mask: n x 64 x 128."""
    n = 1 << (ph * pw)
    idx = np.arange(n, dtype=np.uint32)
    m = np.zeros((n, 64, 128), np.uint8)
    y0, x0 = CORNER_Y - 2, CORNER_X - 2
    for b in range(ph * pw):
        m[:, y0 + b // pw, x0 + b % pw] = ((idx >> b) & 1).astype(np.uint8) * 255
    for k in range(7):
        m[k::7, 2:14, 2:14 + k] = 255
    return m


# ------------------------------------------------------------------ B6
@functools.lru_cache(maxsize=None)
def serpentine(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0, max(w - 3, (w - 1) // TW * TW):] = 255
    right = True
    for y in range(2, h, 2):
        m[y, :] = 255
        m[y - 1, w - 1 if right else 0] = 255
        right = not right
    return m


@functools.lru_cache(maxsize=None)
def corner_link(h, w, d):
    """One component over the corner (64, 32) through a diagonal contact only.  ne: a lone
    pixel at (64, 31) and the body in the tile south-west of it, and so on."""
    m = np.zeros((h, w), np.uint8)
    cy, cx = CORNER_Y, CORNER_X
    py, px, by, bx = {"ne": (cy - 1, cx, cy, cx - 1), "nw": (cy - 1, cx - 1, cy, cx),
                      "se": (cy, cx, cy - 1, cx - 1), "sw": (cy, cx - 1, cy - 1, cx)}[d]
    m[py, px] = 255
    sy, sx = (1 if by >= cy else -1), (1 if bx >= cx else -1)
    # the body: an L along the two tile edges that meet in the corner, clipped to the image,
    # and a second arm two rows on so that it is more than a line
    for t in range(40):
        x = bx + sx * t
        if 0 <= x < w:
            m[by, x] = 255
            if 0 <= by + 2 * sy < h and t >= 1:
                m[by + 2 * sy, x] = 255
        y = by + sy * t
        if 0 <= y < h and t < 25:
            m[y, bx] = 255
    return m


# ------------------------------------------------------------------ B7
def _hook(m, y, x):
    """a 12x12 ring with its top-left pixel at (y, x): contourArea 121"""
    _ring(m, y, x, y + 11, x + 11)


@functools.lru_cache(maxsize=None)
def spiral():
    m = np.zeros((200, 300), np.uint8)
    y0, x0, y1, x1 = 20, 2, 197, 297
    m[y0, x0:x1 + 1] = 255
    while y1 - y0 > 6 and x1 - x0 > 6:
        m[y0:y1 + 1, x1] = 255
        m[y1, x0:x1 + 1] = 255
        y0 += 4
        m[y0:y1 + 1, x0] = 255
        x1 -= 4
        m[y0, x0:x1 + 1] = 255
        y1 -= 4
        x0 += 4
    _hook(m, 9, 2)
    return m


@functools.lru_cache(maxsize=None)
def diagonal():
    m = np.zeros((200, 300), np.uint8)
    for t in range(150):
        m[20 + t, 40 + t] = 255
    _hook(m, 9, 29)  # its corner (20, 40) is the line's first pixel
    return m


@functools.lru_cache(maxsize=None)
def staircase():
    m = np.zeros((200, 300), np.uint8)
    y, x = 14, 14
    while y + 7 < 200 and x + 9 < 300:
        m[y, x:x + 10] = 255
        m[y:y + 8, x + 9] = 255
        y, x = y + 7, x + 9
    _hook(m, 3, 3)
    return m


@functools.lru_cache(maxsize=None)
def window_edge():
    m = np.zeros((200, 300), np.uint8)
    for x in range(20, 257):           # top edge: 8 px on row 63, 8 px on row 64
        m[63 + ((x // 8) & 1), x] = 255
    for x in range(24, 257, 8):
        m[63:65, x - 1:x + 1] = 255    # joins of the two rows
    for y in range(63, 191):           # right edge: 8 px on column 255, 8 px on column 256
        m[y, 255 + ((y // 8) & 1)] = 255
    for y in range(64, 191, 8):
        m[y - 1:y + 1, 255:257] = 255
    m[190, 20:257] = 255
    m[63:191, 20] = 255
    return m


# ------------------------------------------------------------------ B8 / B9
def comb(h, w):
    """Stacked combs: a spine down column 1, a full row every 4th row, 1-px teeth on every
    second column beneath it, and a 12x12 ring on the spine's foot for the area.  For even w
    and h = 4 R the border has R (w + 2) + 4 vertices."""
    m = np.zeros((h + 13, max(w, 16)), np.uint8)
    m[0:h, 1] = 255
    for y in range(0, h - 2, 4):
        m[y, 1:w] = 255
        m[y + 1, 3:w:2] = 255
    _hook(m, h, 1)
    return m


# name -> (h, w, vertices of its one contour)
COMBS = {
    "comb_a": (40, 100, PTS_LDS),       # the longest contour k_ct_shapes stages in LDS
    "comb_b": (28, 144, PTS_LDS + 2),   # the shortest it can read from global memory
    "comb_c": (184, 176, STAGE),        # fills k_ct_trace's staging area
    "comb_d": (156, 208, STAGE + 2),    # followed a second time
    "comb_e": (202, 260, 13104),
}


@functools.lru_cache(maxsize=None)
def comb_case(name):
    h, w, _ = COMBS[name]
    return comb(h, w)


@functools.lru_cache(maxsize=None)
def regrow():
    one = comb(116, 200)  # 5862 vertices, x 15 = 87 930
    th, tw = one.shape[0] + 4, one.shape[1] + 2
    m = np.zeros((3 * th, 5 * tw), np.uint8)
    for k in range(15):
        y, x = (k // 5) * th, (k % 5) * tw
        m[y:y + one.shape[0], x:x + one.shape[1]] = one
    return m


# ------------------------------------------------------------------ the catalogue
def single_cases():
    """name -> builder of one h x w mask (everything but the B5 batches)"""
    c = {"rej_grid": rej_grid, "rej_straddle_few": lambda: rej_straddle(False),
         "rej_straddle_many": lambda: rej_straddle(True), "restarts": restarts, "spiral": spiral,
         "diagonal": diagonal, "staircase": staircase, "window_edge": window_edge, "regrow": regrow}
    for n in (64, 65, 66):
        c[f"rej_{n}"] = functools.partial(rej_n, n)
    for w in WIDE:
        c[f"wide_rej_{w}"] = functools.partial(wide_rej, w)
        c[f"far_{w}"] = functools.partial(far, w)
    for h, w in SIZES:
        c[f"serpentine_{h}x{w}"] = functools.partial(serpentine, h, w)
        for d in ("ne", "nw", "se", "sw"):
            c[f"corner_{d}_{h}x{w}"] = functools.partial(corner_link, h, w, d)
    for name in COMBS:
        c[name] = functools.partial(comb_case, name)
    return c


SINGLE = single_cases()

# exact number of rejected components (8-connected components - contours) where the row states one
REJECTED = {"rej_grid": 462, "rej_64": 64, "rej_65": 65, "rej_66": 66, "rej_straddle_few": 7,
            "rej_straddle_many": 77, "restarts": 8}


# ------------------------------------------------------------------ counters (CPU)
def components(mask):
    """(label image, count) under 8-connectivity"""
    from scipy import ndimage

    return ndimage.label(mask != 0, structure=np.ones((3, 3)))


def first_pixels(mask):
    """set of (x, y): the raster-first pixel of every 8-connected component"""
    from scipy import ndimage

    lab, k = components(mask)
    if not k:
        return set()
    pos = ndimage.minimum(np.arange(mask.size).reshape(mask.shape), lab, np.arange(1, k + 1))
    w = mask.shape[1]
    return {(int(p) % w, int(p) // w) for p in np.atleast_1d(pos)}


def counters(mask, contours):
    """What a mask reaches, from its contour list: components, contours, rejected, the longest
    contour, all vertices, contours not started at a component's first pixel."""
    _, k = components(mask)
    fp = first_pixels(mask)
    return {"components": k, "contours": len(contours), "rejected": k - len(contours),
            "longest": max((len(c) for c in contours), default=0), "vertices": sum(len(c) for c in contours),
            "off_first": sum((int(c[0][0]), int(c[0][1])) not in fp for c in contours)}


def far_lookups(mask):
    """First pixels at x >= 4032 whose row has foreground left of 3968 and none in 3968 .. x - 1:
    their lnbd, if it is a mark at all, is outside the second window (a lower bound of
    pix_is_right_mark's calls: unmarked non-first pixels ask as well)."""
    n = 0
    for x, y in first_pixels(mask):
        if x >= WIN0 and not mask[y, LANE0:x].any() and mask[y, :LANE0].any():
            n += 1
    return n


def dp_depth(pts, eps):
    """OpenCV's closed iterative Douglas-Peucker restated (contours.cpp dp_vertex_count) ->
    (largest slice-stack depth in pairs, points emitted before the collinear clean-up, vertex
    count after it)."""
    p = np.asarray(pts, np.int64)
    count = len(p)
    if count == 0:
        return 0, 0, 0
    eps2 = eps * eps
    pos = rs = 0
    le_eps = False
    for _ in range(3):
        pos = (pos + rs) % count
        d = ((np.roll(p, -pos, axis=0)[1:] - p[pos]) ** 2).sum(1)
        dmax = int(d.max()) if len(d) else 0
        if dmax > 0:
            rs = int(np.argmax(d)) + 1
        le_eps = dmax <= eps2
    if le_eps:
        return 0, 1, 1
    a = pos % count
    b = (rs + a) % count
    stack = [(b, a), (a, b)]
    deepest, out = 2, []
    while stack:
        s, e = stack.pop()
        m = (e - s - 1) % count
        ok, split = True, 0
        if m > 0:
            dx, dy = p[e] - p[s]
            idx = (s + 1 + np.arange(m)) % count
            d = np.abs((p[idx, 1] - p[s, 1]) * dx - (p[idx, 0] - p[s, 0]) * dy)
            dmax = int(d.max())
            if dmax > 0:
                split = int(idx[int(np.argmax(d))])
            ok = float(dmax) * float(dmax) <= eps2 * (float(dx) * float(dx) + float(dy) * float(dy))
        if ok:
            out.append((int(p[s, 0]), int(p[s, 1])))
        else:
            stack += [(split, e), (s, split)]
            deepest = max(deepest, len(stack))
    return deepest, len(out), _dp_cleanup(out, eps2)


def _dp_cleanup(dst, eps2):
    """the closed contour's pass over [almost] collinear points -> the final vertex count"""
    cnt = newc = len(dst)
    dst = list(dst)
    pos = cnt - 1

    def rd():
        nonlocal pos
        v = dst[pos]
        pos = pos + 1 if pos + 1 < cnt else 0
        return v

    sx, sy = rd()
    wpos = pos
    px, py = rd()
    i = 0
    while i < cnt and newc > 2:
        qx, qy = rd()
        dx, dy = float(qx - sx), float(qy - sy)
        d = abs((px - sx) * dy - (py - sy) * dx)
        sip = float(px - sx) * (qx - px) + float(py - sy) * (qy - py)
        if d * d <= 0.5 * eps2 * (dx * dx + dy * dy) and dx != 0 and dy != 0 and sip >= 0:
            newc -= 1
            sx, sy = qx, qy
            dst[wpos] = (qx, qy)
            wpos = wpos + 1 if wpos + 1 < cnt else 0
            px, py = rd()
            i += 2
            continue
        sx, sy = px, py
        dst[wpos] = (px, py)
        wpos = wpos + 1 if wpos + 1 < cnt else 0
        px, py = qx, qy
        i += 1
    return newc
