"""Small directed cases for the preprocessing kernels: cvresize.hip (cv2.resize), resize.hip
(Pillow LANCZOS / reduce / thumbnail) and text.hip (Otsu binary).

tests/test_resize_case_inputs.py checks, on the CPU, that the tables reach the branches they
claim (through the restatements below) and checks the oracle on them against Pillow itself and
against a second NumPy statement of cv2.resize; tests/test_gpu_resize_cases.py runs the device
on the same cases, bit-exact.  Images and expected values are computed once per case and shared
(``functools.lru_cache``): callers must not modify them.

``cv_plan`` restates cv_resize_plan's classification (cvresize.hip), ``pil_plan`` Pillow's
precompute_coeffs for LANCZOS as resize_lanczos_n uses it (llfe_resize.cpp) -- for the box as
given and for the box rounded to float32, which is what Pillow's C code receives --, and
``thumb_plan`` the size rule, reduce factors and box of Image.thumbnail.  ``np_cv_resize`` is
the NumPy statement of cv2.resize that tests/test_oracle_kat.py also uses.

cv2 cases (expected: the oracle's cv_resize), (h, w) -> (oh, ow), the smallest shapes that reach:

  COPY        (5, 7) -> (5, 7), each interpolation
  AREA_FAST   (6, 10) -> (3, 5): exact 2x2, (s + 2) >> 2 for cn 1, 3, 4, rounded float for cn 2 (the
              forms differ where s % 8 == 2); as LINEAR too (the exact-2x rule makes it AREA)
              (9, 12) -> (3, 4) 3x3; (8, 9) -> (4, 3) factors 3 and 2; (7, 9) -> (1, 1) factors 9 and 7
  AREA        (7, 11) -> (3, 4); (9, 7) -> (3, 2) integer in y, fractional in x; (13, 5) -> (12, 4)
              scale just above 1; (1, 9) -> (1, 4) and (9, 1) -> (4, 1) one-row / one-column sources
  GENERIC 2   LINEAR (6, 10) -> (3, 7): 2x in one axis stays generic; (18, 26) -> (7, 13) down;
              (5, 7) -> (13, 17) up (sx < 0 clamp, xmin > 0, xmax < ow); (4, 1) -> (9, 5): xmax == 0,
              every column the single-tap arm; (1, 4) -> (5, 9): h == 1
              (7, 11) -> 4 rows of 6, 8, 9, 15, 16, 17, 24, 27 bytes: (x_vec, tail) = (0, 6), (0, 8),
              (8, 1), (8, 7), (16, 0), (16, 1), (16, 8), (24, 3)
              AREA (5, 7) -> (13, 17), (12, 10) -> (6, 25), (10, 12) -> (25, 6): area_mode, pure
              upscale and both mixed directions
  GENERIC 4   CUBIC up and down with rows of 9, 51, 10 and 52 bytes (x_vec 0 / 48); (1, 1) -> (4, 5);
              (6, 1) -> (9, 6) w == 1 (x_vec 16, tail 8); (1, 6) -> (3, 20) h == 1 (x_vec 16, tail 4)
              (8, 40) -> (4, 20) on rows built to tie: the float form of the vector loop rounds
              to even, the fixed-point form of the tail rounds up (``cubic_ties``)
  GENERIC 8   LANCZOS4 from sources 1, 2, 3 and 5 pixels wide and high (taps clamp on both sides at
              once); (5, 7) -> (13, 17); (18, 26) -> (7, 13)

Every cv2 case runs on three images: uniform random bytes, random 0 / 255 (overshoot and
saturation of CUBIC and LANCZOS4, whose sum is kept mod 2^32, and the largest operands of the
LINEAR vector path, 255 * 2048 >> 4 = 32640: with u8 sources its 16-bit clamps never bind) and a
one-pixel checkerboard shifted by one per channel.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

DBL_EPS = 2.220446049250313e-16
KS = {"linear": 2, "area": 2, "cubic": 4, "lanczos4": 8}


# --------------------------------------------------------------------------- images
@functools.lru_cache(maxsize=None)
def images(h, w, cn, seed=0):
    """(rand, sat, checker): three h x w x cn uint8 images (read-only)."""
    rand = np.random.default_rng([11, seed, h, w, cn]).integers(0, 256, (h, w, cn), dtype=np.uint8)
    sat = (np.random.default_rng([12, seed, h, w, cn]).integers(0, 2, (h, w, cn)) * 255).astype(np.uint8)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(cn), indexing="ij")
    checker = (((y + x + c) & 1) * 255).astype(np.uint8)
    out = (rand, sat, np.ascontiguousarray(checker))
    for a in out:
        a.setflags(write=False)
    return out


IMAGE_KINDS = ("rand", "sat", "checker", "directed")  # (the fourth only where a case has one)


# --------------------------------------------------------------------------- cv2.resize
class CvPlan(NamedTuple):
    kind: str  # COPY / AREA_FAST / AREA / GENERIC
    interp: str  # after the exact-2x rule
    fx: float  # scale_x (an int for AREA_FAST)
    fy: float
    ks: int = 0
    xmin: int = 0
    xmax: int = 0
    x_vec: int = 0
    tail: int = 0  # ow * cn - x_vec
    area_mode: bool = False


def cv_tap(d, scale, inv, area_mode):
    """Source index and float32 phase of output index d, before any clamp."""
    if not area_mode:
        f = np.float32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = np.float32(f - np.float32(s))
    else:
        s = math.floor(d * scale)
        f = np.float32((d + 1) - (s + 1) * inv)
        f = np.float32(0) if f <= 0 else np.float32(f - np.float32(math.floor(f)))
    return s, f


def cv_x_vec(width, ks):
    """Stop of the vertical pass's 128-bit vector loops: steps of 16, LINEAR then steps of 8."""
    xv = 0
    while xv <= width - 16:
        xv += 16
    if ks == 2:
        while xv < width - 8:
            xv += 8
    return xv


def cv_plan(h, w, cn, oh, ow, interp):
    """cv_resize_plan's classification (cvresize.hip) for a given dsize."""
    if (oh, ow) == (h, w):
        return CvPlan("COPY", interp, 1, 1)
    inv_x, inv_y = ow / w, oh / h
    scale_x, scale_y = 1.0 / inv_x, 1.0 / inv_y
    ix, iy = round(scale_x), round(scale_y)
    fast = abs(scale_x - ix) < DBL_EPS and abs(scale_y - iy) < DBL_EPS
    if interp == "linear" and fast and ix == 2 and iy == 2:
        interp = "area"
    if interp == "area" and scale_x >= 1 and scale_y >= 1:
        if fast:
            return CvPlan("AREA_FAST", interp, ix, iy)
        return CvPlan("AREA", interp, scale_x, scale_y)
    ks = KS[interp]
    area_mode = interp == "area"
    xmin, xmax = 0, ow
    for dx in range(ow):
        sx, _ = cv_tap(dx, scale_x, inv_x, area_mode)
        if sx < ks // 2 - 1:
            xmin = dx + 1
            if sx < 0 and ks == 2:
                sx = 0  # LINEAR's clamp comes before the right-hand test
        if sx + ks // 2 >= w:
            xmax = min(xmax, dx)
    xv = cv_x_vec(ow * cn, ks)
    return CvPlan("GENERIC", interp, scale_x, scale_y, ks, xmin, xmax, xv, ow * cn - xv, area_mode)


def np_area_tab(ssize, dsize, scale):
    tab = []
    for dx in range(dsize):
        f1 = dx * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            tab.append((dx, s1 - 1, np.float32((s1 - f1) / cell)))
        for s in range(s1, s2):
            tab.append((dx, s, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            tab.append((dx, s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
    return tab


def np_lanczos4(x):
    x = np.float32(x)
    s45 = 0.70710678118654752440084436210485
    cs = [(1, 0), (-s45, -s45), (0, 1), (s45, -s45), (-1, 0), (s45, s45), (0, -1), (-s45, s45)]
    y0 = -float(np.float32(x + np.float32(3))) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c = []
    tot = np.float32(0)
    for i in range(8):
        yi = np.float32(np.float32(x + np.float32(3)) - np.float32(i))
        if abs(yi) >= np.float32(1e-6):
            y = -float(yi) * math.pi * 0.25
            v = np.float32((cs[i][0] * s0 + cs[i][1] * c0) / (y * y))
        else:
            v = np.float32(1e30)
        c.append(v)
        tot = np.float32(tot + v)
    inv = np.float32(np.float32(1) / tot)
    return [np.float32(v * inv) for v in c]


def s16(v):
    return int(np.clip(np.rint(np.float32(v)), -32768, 32767))


def np_cv_resize(img, ow, oh, interp):
    """cv2.resize(img, (ow, oh), INTER_<interp>) for "area", "linear" and "lanczos4" in NumPy:
    float32 scalars for OpenCV's float steps, int64 for its fixed point (reduced mod 2^32 where
    OpenCV's int accumulator is).  Down- and upscales: LINEAR's sx < 0 and sx >= w - 1 clamps
    (columns only: rows are clamped when they are read, their phase stays) and AREA's upscale
    rule for sx / fx (area_mode)."""
    h, w, cn = img.shape
    inv_x, inv_y = ow / w, oh / h
    scale_x, scale_y = 1.0 / inv_x, 1.0 / inv_y
    ix, iy = int(round(scale_x)), int(round(scale_y))
    fast = abs(scale_x - ix) < DBL_EPS and abs(scale_y - iy) < DBL_EPS
    if (oh, ow) == (h, w):
        return img.copy()
    if interp == "linear" and fast and ix == 2 and iy == 2:
        interp = "area"
    if interp == "area" and scale_x >= 1 and scale_y >= 1:
        if fast:
            out = np.zeros((oh, ow, cn), np.uint8)
            for dy in range(oh):
                for dx in range(ow):
                    blk = img[dy * iy:(dy + 1) * iy, dx * ix:(dx + 1) * ix].astype(np.int64)
                    s = blk.sum(axis=(0, 1))
                    if ix == 2 and iy == 2 and cn != 2:  # the vector form exists for cn 1, 3, 4 only
                        out[dy, dx] = (s + 2) >> 2
                    else:
                        out[dy, dx] = np.clip(np.rint(s.astype(np.float32) * np.float32(1.0 / np.float32(ix * iy))),
                                              0, 255)
            return out
        S = img.astype(np.float32)
        buf = np.zeros((h, ow, cn), np.float32)
        for dx, sx, a in np_area_tab(w, ow, scale_x):
            buf[:, dx] = buf[:, dx] + S[:, sx] * a
        acc = np.zeros((oh, ow, cn), np.float32)
        for dy, sy, b in np_area_tab(h, oh, scale_y):
            acc[dy] = acc[dy] + b * buf[sy]
        return np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    ks = 8 if interp == "lanczos4" else 2
    area_mode = interp == "area"

    def coeffs(d, scale, inv, n, columns):
        s, f = cv_tap(d, scale, inv, area_mode)
        if ks == 2 and columns:
            if s < 0:
                s, f = 0, np.float32(0)
            if s >= n - 1:
                s, f = n - 1, np.float32(0)
        c = np_lanczos4(f) if ks == 8 else [np.float32(1) - f, f]
        return s, [s16(np.float32(v * np.float32(2048))) for v in c]

    xs = [coeffs(dx, scale_x, inv_x, w, True) for dx in range(ow)]
    ys = [coeffs(dy, scale_y, inv_y, h, False) for dy in range(oh)]
    I = img.astype(np.int64)
    # horizontal pass for every source row: (h, ow, cn)
    hor = np.zeros((h, ow, cn), np.int64)
    for dx, (sx, a) in enumerate(xs):
        for j in range(ks):
            col = min(max(sx - (ks // 2 - 1) + j, 0), w - 1)
            hor[:, dx] += I[:, col] * a[j]
    width = ow * cn
    x_vec = cv_x_vec(width, 2)
    out = np.zeros((oh, ow * cn), np.int64)
    for dy, (sy, b) in enumerate(ys):
        rows = [hor[min(max(sy - (ks // 2 - 1) + k, 0), h - 1)].reshape(-1) for k in range(ks)]
        if ks == 8:
            v = sum(r * bk for r, bk in zip(rows, b)) + (1 << 21)
            v = ((v + (1 << 31)) % (1 << 32)) - (1 << 31)  # a 32-bit accumulator
            out[dy] = v >> 22
        else:
            scal = (rows[0] * b[0] + rows[1] * b[1] + (1 << 21)) >> 22
            s0, s1 = (np.clip(r >> 4, -32768, 32767) for r in rows)
            t = ((s0 * b[0]) >> 16) + ((s1 * b[1]) >> 16)
            vec = (np.clip(t, -32768, 32767) + 2) >> 2
            idx = np.arange(width)
            out[dy] = np.where(idx < x_vec, vec, scal)
    return np.clip(out, 0, 255).astype(np.uint8).reshape(oh, ow, cn)


class CvCase(NamedTuple):
    group: str
    h: int
    w: int
    cn: int
    oh: int
    ow: int
    interp: str

    @property
    def id(self):
        return f"{self.group}-{self.interp}-{self.h}x{self.w}x{self.cn}-to-{self.oh}x{self.ow}"


def _cv(group, interp, rows):
    return [CvCase(group, h, w, cn, oh, ow, interp) for (h, w, cn, oh, ow) in rows]


# rows of (x_vec, tail) for the LINEAR vector stop: output rows of ow * cn bytes
VEC_ROWS = {6: (0, 6), 8: (0, 8), 9: (8, 1), 15: (8, 7), 16: (16, 0), 17: (16, 1), 24: (16, 8), 27: (24, 3)}

CV_CASES = (
    [CvCase("copy", 5, 7, cn, 5, 7, interp)
     for cn, interp in ((1, "linear"), (2, "cubic"), (3, "area"), (4, "lanczos4"))]
    + _cv("fast2x2", "area", [(6, 10, 1, 3, 5), (6, 10, 2, 3, 5), (6, 10, 3, 3, 5), (6, 10, 4, 3, 5)])
    + _cv("fast2x2", "linear", [(6, 10, 2, 3, 5), (6, 10, 3, 3, 5)])
    + _cv("fast", "area", [(9, 12, 3, 3, 4), (9, 12, 2, 3, 4), (8, 9, 1, 4, 3), (7, 9, 4, 1, 1)])
    + _cv("one_axis_2x", "linear", [(6, 10, 3, 3, 7)])
    + _cv("area_tab", "area", [(7, 11, 3, 3, 4), (9, 7, 1, 3, 2), (13, 5, 4, 12, 4), (1, 9, 2, 1, 4), (9, 1, 3, 4, 1)])
    + _cv("generic2", "linear", [(18, 26, 3, 7, 13), (5, 7, 1, 13, 17), (5, 7, 4, 13, 17), (4, 1, 2, 9, 5),
                                 (1, 4, 3, 5, 9)])
    + _cv("vec_stop", "linear", [(7, 11, 2, 4, 3), (7, 11, 4, 4, 2), (7, 11, 3, 4, 3), (7, 11, 3, 4, 5),
                                 (7, 11, 4, 4, 4), (7, 11, 1, 4, 17), (7, 11, 4, 4, 6), (7, 11, 3, 4, 9)])
    + _cv("area_mode", "area", [(5, 7, 3, 13, 17), (12, 10, 1, 6, 25), (10, 12, 4, 25, 6), (12, 10, 2, 6, 25)])
    + _cv("generic4", "cubic", [(5, 4, 1, 11, 9), (5, 7, 3, 13, 17), (18, 26, 2, 7, 5), (18, 26, 4, 7, 13),
                                (1, 1, 3, 4, 5), (6, 1, 4, 9, 6), (1, 6, 1, 3, 20)])
    + _cv("cubic_ties", "cubic", [(8, 40, 1, 4, 20)])
    + _cv("generic8", "lanczos4", [(1, 1, 3, 3, 4), (2, 2, 1, 5, 3), (3, 3, 4, 7, 8), (5, 5, 2, 4, 9), (1, 5, 3, 2, 9),
                                   (5, 1, 1, 9, 2), (2, 3, 2, 1, 1), (5, 7, 3, 13, 17), (18, 26, 3, 7, 13),
                                   (18, 26, 4, 7, 13)])
)


def cubic_ties():
    """8 x 40 grey rows for CUBIC -> (4, 20): at exactly 2x every phase is 0.5, the taps are
    (-192, 1216, 1216, -192) / 2048 and, the rows being constant, the horizontal pass gives
    2048 v.  Output row 1 sees v = (0, 20, 28, 0): 19 * 48 / 32 = 28.5; row 2 sees (28, 0, 7, 11):
    (-84 + 133 - 33) / 32 = 0.5.  On such ties the float form of the 16 vector-loop bytes rounds to
    even (28, 0) and the fixed-point form of the 4 tail bytes rounds up (29, 1)."""
    v = np.array([0, 0, 20, 28, 0, 7, 11, 0], np.uint8)
    return np.ascontiguousarray(np.repeat(v[:, None], 40, 1)[:, :, None])


def cv_images(case):
    """The case's images in the order of IMAGE_KINDS."""
    x = images(case.h, case.w, case.cn)
    return x + (cubic_ties(),) if case.group == "cubic_ties" else x


def _orc():
    from oracle import oracle

    oracle.lib()
    return oracle


@functools.lru_cache(maxsize=None)
def cv_expected(case):
    """The oracle's cv_resize of the case's three images (read-only)."""
    O = _orc()
    out = tuple(O.cv_resize(x, case.ow, case.oh, case.interp) for x in cv_images(case))
    for a in out:
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------- Pillow LANCZOS
class PilPlan(NamedTuple):
    bounds_h: np.ndarray  # (ow, 2): xmin, count
    kk_h: np.ndarray  # (ow, ksize) 22-bit coefficients
    bounds_v: np.ndarray  # (oh, 2), before the yfirst shift
    kk_v: np.ndarray
    need_h: bool
    need_v: bool
    yfirst: int
    ylast: int


def _lanczos(x):
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v

    return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def pil_coeffs(in_size, in0, in1, out_size, float_args=False):
    """precompute_coeffs (libImaging/Resample.c) for LANCZOS, then normalize_coeffs_8bpc:
    (bounds (out, 2), coefficients (out, ksize)) with sequential double sums.  float_args: in0 and
    in1 are Pillow's float arguments, which it subtracts as floats before widening."""
    scale = (float(np.float32(in1) - np.float32(in0)) if float_args else in1 - in0) / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        for x, v in enumerate(k):
            v = v * (1 << 22)
            kk[xx, x] = int(-0.5 + v) if v < 0 else int(0.5 + v)
        bounds[xx] = xmin, xmax
    return bounds, kk


def _pil_plan_one(h, w, oh, ow, box, float_args):
    bx0, by0, bx1, by1 = box
    bh, kh = pil_coeffs(w, bx0, bx1, ow, float_args)
    bv, kv = pil_coeffs(h, by0, by1, oh, float_args)
    need_h = ow != w or bx0 != 0 or bx1 != ow
    need_v = oh != h or by0 != 0 or by1 != oh
    return PilPlan(bh, kh, bv, kv, bool(need_h), bool(need_v), int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1]))


def pil_plan(h, w, oh, ow, box=None):
    """{"f64": plan for the box as given (doubles), "f32": plan for the box rounded to float32}."""
    box = (0.0, 0.0, float(w), float(h)) if box is None else tuple(float(v) for v in box)
    box32 = tuple(float(np.float32(v)) for v in box)
    return {"f64": _pil_plan_one(h, w, oh, ow, box, False), "f32": _pil_plan_one(h, w, oh, ow, box32, True)}


def coeffs_differ(h, w, oh, ow, box):
    """22-bit coefficients (and bounds) that differ between the double and the float32 box."""
    p = pil_plan(h, w, oh, ow, box)
    a, b = p["f64"], p["f32"]
    n = 0
    for u, v in ((a.kk_h, b.kk_h), (a.kk_v, b.kk_v), (a.bounds_h, b.bounds_h), (a.bounds_v, b.bounds_v)):
        n += int((u != v).sum())
    return n


class LanczosCase(NamedTuple):
    name: str
    h: int
    w: int
    ch: int
    oh: int
    ow: int
    box: tuple | None  # (x0, y0, x1, y1) in source pixels

    @property
    def id(self):
        return f"{self.name}-{self.h}x{self.w}x{self.ch}-to-{self.oh}x{self.ow}"


LANCZOS_CASES = (
    LanczosCase("both", 30, 40, 3, 13, 17, None),
    LanczosCase("both_ch1", 23, 31, 1, 9, 14, (1.5, 2.25, 30.0, 20.75)),
    LanczosCase("h_only", 20, 50, 3, 20, 23, (3.5, 0.0, 45.25, 20.0)),
    LanczosCase("v_only", 50, 20, 2, 23, 20, (0.0, 3.5, 20.0, 45.25)),
    LanczosCase("neither", 12, 9, 2, 12, 9, None),
    LanczosCase("neither_full_box", 12, 9, 4, 12, 9, (0.0, 0.0, 9.0, 12.0)),
    LanczosCase("yfirst_h", 120, 90, 3, 20, 33, (0.0, 60.0, 90.0, 100.0)),
    LanczosCase("yfirst_no_h", 120, 90, 4, 20, 90, (0.0, 60.0, 90.0, 100.0)),
    LanczosCase("non_dyadic", 120, 200, 3, 40, 70, (10.1, 3.3, 190.7, 117.9)),
    LanczosCase("upscale", 9, 11, 3, 25, 31, None),
    LanczosCase("upscale_box", 9, 11, 1, 25, 31, (2.2, 1.1, 9.9, 8.3)),
    LanczosCase("one_by_one", 13, 17, 4, 1, 1, None),
    LanczosCase("w1", 9, 1, 1, 4, 3, None),
    LanczosCase("h1", 1, 9, 2, 3, 4, None),
)


def _pil_planes(img, fn):
    """fn(PIL image) per "RGB" image (ch == 3) or per "L" plane, stacked (Pillow premultiplies
    alpha for "RGBA" / "LA", which the kernels do not and the product never asks for)."""
    from PIL import Image

    img = np.asarray(img)
    if img.shape[2] == 3:
        return np.array(fn(Image.fromarray(img)))
    planes = [np.ascontiguousarray(img[:, :, c]) for c in range(img.shape[2])]
    return np.stack([np.array(fn(Image.fromarray(p))) for p in planes], -1)


@functools.lru_cache(maxsize=None)
def lanczos_expected(case):
    """Pillow's Image.resize((ow, oh), LANCZOS, box) of the case's three images."""
    from PIL import Image

    out = tuple(_pil_planes(x, lambda im: im.resize((case.ow, case.oh), Image.Resampling.LANCZOS, box=case.box))
                for x in images(case.h, case.w, case.ch))
    for a in out:
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------- Pillow reduce
class ReduceCase(NamedTuple):
    h: int
    w: int
    ch: int
    fx: int
    fy: int

    @property
    def id(self):
        return f"{self.h}x{self.w}x{self.ch}-by-{self.fx}x{self.fy}"


_FACTORS = ((1, 3), (3, 1), (2, 2), (3, 3), (5, 2), (7, 7), (1, 2), (2, 1), (4, 4), (5, 5))  # (fx, fy)
REDUCE_CASES = tuple(
    [ReduceCase(fy * 4, fx * 5, 1 if i % 2 else 4, fx, fy) for i, (fx, fy) in enumerate(_FACTORS)]  # no remainder
    + [ReduceCase(fy * 4 + 1, fx * 5 + max(fx - 1, 1), 4 if i % 2 else 1, fx, fy)  # a remainder in each axis
       for i, (fx, fy) in enumerate(_FACTORS)]
    + [ReduceCase(3, 4, 4, 5, 7), ReduceCase(3, 4, 1, 5, 7),  # a factor larger than the dimension
       ReduceCase(33, 100, 1, 50, 16), ReduceCase(33, 100, 4, 50, 16)]
)


@functools.lru_cache(maxsize=None)
def reduce_expected(case):
    out = tuple(_pil_planes(x, lambda im: im.reduce((case.fx, case.fy))) for x in images(case.h, case.w, case.ch))
    for a in out:
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------- Pillow thumbnail
class ThumbPlan(NamedTuple):
    ow: int
    oh: int
    fx: int
    fy: int
    rem_x: int  # w % fx: columns of the last, narrower reduce cell
    rem_y: int
    box: tuple | None  # box of the resize after the reduce pre-pass; None without one
    resized: bool


def thumb_plan(h, w, max_w, max_h, reducing_gap=2.0):
    """Image.thumbnail((max_w, max_h), LANCZOS): the size rule (preserve_aspect_ratio), the
    reduce factors of Image.resize's reducing_gap and the box it leaves."""
    x, y = math.floor(max_w), math.floor(max_h)
    if x >= w and y >= h:
        return ThumbPlan(w, h, 1, 1, 0, 0, None, False)
    aspect = w / h

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    if (x, y) == (w, h):
        return ThumbPlan(w, h, 1, 1, 0, 0, None, False)
    fx = int(w / x / reducing_gap) or 1
    fy = int(h / y / reducing_gap) or 1
    box = (0.0, 0.0, w / fx, h / fy) if fx > 1 or fy > 1 else None
    return ThumbPlan(x, y, fx, fy, w % fx, h % fy, box, True)


class ThumbCase(NamedTuple):
    h: int
    w: int
    ch: int
    max_w: int
    max_h: int
    seed: int
    float_box: bool = False  # the box rounded to float32 gives other coefficients than the double box

    @property
    def id(self):
        return f"{self.h}x{self.w}x{self.ch}-into-{self.max_w}x{self.max_h}-seed{self.seed}"


FLOAT_BOX_SHAPES = ((500, 1601, 256, 256), (1300, 650, 200, 200), (1001, 1003, 160, 160))  # factor (3, 3) each
THUMB_CASES = tuple(
    [ThumbCase(h, w, 3, mw, mh, seed, True) for (h, w, mw, mh) in FLOAT_BOX_SHAPES for seed in (0, 1, 2)]
    + [ThumbCase(37, 401, 3, 50, 50, 0, True),  # factor (4, 3)
       ThumbCase(37, 401, 1, 50, 50, 1, True),
       ThumbCase(37, 401, 4, 50, 50, 2, True),
       ThumbCase(33, 100, 3, 1, 1, 0),  # factor (50, 16)
       ThumbCase(9, 1000, 3, 100, 2, 0),  # factor (5, 4)
       ThumbCase(20, 30, 3, 64, 64, 0),  # fits: a copy
       ThumbCase(20, 30, 4, 30, 20, 0),
       ThumbCase(50, 70, 3, 32, 32, 0),  # resized without the pre-pass
       ThumbCase(50, 70, 1, 32, 32, 1)]
)
THUMB_FACTORS = {(500, 1601, 256, 256): (3, 3), (1300, 650, 200, 200): (3, 3), (1001, 1003, 160, 160): (3, 3),
                 (37, 401, 50, 50): (4, 3), (33, 100, 1, 1): (50, 16), (9, 1000, 100, 2): (5, 4),
                 (20, 30, 64, 64): (1, 1), (20, 30, 30, 20): (1, 1), (50, 70, 32, 32): (1, 1)}
THUMB_SIZES = {(500, 1601, 256, 256): (80, 256), (1300, 650, 200, 200): (200, 100), (1001, 1003, 160, 160): (160, 160)}
BATCH_CASE = (1300, 650, 200, 200, (0, 1, 2))  # three images of one float-box shape


@functools.lru_cache(maxsize=None)
def thumb_image(h, w, ch, seed):
    x = np.random.default_rng(seed).integers(0, 256, (h, w, ch), dtype=np.uint8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def thumb_expected(case):
    """Pillow's Image.thumbnail((max_w, max_h), LANCZOS) of thumb_image(case)."""
    from PIL import Image

    def thumb(im):
        im.thumbnail((case.max_w, case.max_h), Image.Resampling.LANCZOS)
        return im

    out = _pil_planes(thumb_image(case.h, case.w, case.ch, case.seed), thumb)
    out.setflags(write=False)
    return out


# --------------------------------------------------------------------------- text binary
TEXT_GRID = 2048 * 256  # pixels one trip of text.hip's grid-stride loops covers


def _gray_to_channels(g, c):
    """A c-channel image whose BGR2GRAY is g ((v, v, v) maps to v; the fourth channel is ignored)."""
    if c == 1:
        return g[:, :, None].copy()
    x = np.repeat(g[:, :, None], c, 2)
    if c == 4:
        x[:, :, 3] = 255 - g
    return np.ascontiguousarray(x)


def _two_valued(h, w, n_high, lo, hi):
    g = np.full(h * w, lo, np.uint8)
    g[np.random.default_rng([13, n_high]).permutation(h * w)[:n_high]] = hi
    return g.reshape(h, w)


@functools.lru_cache(maxsize=None)
def text_cases():
    """name -> image.  51 x 100 = 5100 = 255 * 20 pixels: mean(binary) > 127 <=> ones > 2540."""
    cases = {
        "constant": np.full((40, 120, 3), 128, np.uint8),
        # every split in [10, 199] ties; the first maximum, 10, is the threshold
        "tie": _gray_to_channels(np.tile(np.array([10] * 30 + [200] * 70, np.uint8), (30, 1)), 1),
        "ones_2540": _gray_to_channels(_two_valued(51, 100, 2540, 50, 200), 3),  # not inverted
        "ones_2541": _gray_to_channels(_two_valued(51, 100, 2541, 50, 200), 4),  # inverted
    }
    r = np.random.default_rng(14)
    big = r.integers(0, 256, (600, 900, 1), dtype=np.uint8)
    big[200:400, 225:450] //= 4
    cases["second_trip"] = big  # 540 000 pixels, no upscale
    up = r.integers(0, 256, (4, 300, 3), dtype=np.uint8)
    up[1:3, 75:150] //= 4
    cases["upscaled_second_trip"] = up  # x 25: 100 x 7500 = 750 000 pixels
    for a in cases.values():
        a.setflags(write=False)
    return cases


TEXT_NAMES = ("constant", "tie", "ones_2540", "ones_2541", "second_trip", "upscaled_second_trip")


@functools.lru_cache(maxsize=None)
def text_expected(name):
    out, t = _orc().text_binary(text_cases()[name])
    out.setflags(write=False)
    return out, t
