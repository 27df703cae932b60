"""Shapes and images for the seams of the row-streaming stencil (stencil_stream.hip).

tests/test_stencil_seam_inputs.py checks, on the CPU, the geometry this table claims and that
the images reach the threshold and NMS ties; tests/test_gpu_stencil_seams.py runs the three
stage entry points (and process() on the shapes marked +) on them against the oracle.
Images and expected values are computed once per shape and shared (``functools.lru_cache``):
callers must not modify them.

One wave owns a strip of 240 output columns (a 256-column window with an 8-column halo) and a
segment of seg_rows = ceil(H / ceil(H / 216)) rows; its register rings are indexed by the row
step modulo 12, so a segment that starts at row ya starts at ring phase ya % 12 and the
REPLICATE rows t >= H enter at phase H % 12.  ``geometry`` restates stream_geometry.

  group  shapes (+ = process() too)                       n     seam
  G1     H in 1..7, 13 x W in 1..12                       3     reflect101 bouncing more than once (W < 8, H < 6);
                                                                one partial strip, byte loads (W % 4 != 0)
  G2     13 x 236 239 240 241+ 243 244+ 248 252           3, 5  last strip of 1..12 columns; W = 240, 480, 720
         476 480+ 481 484 488+ 492 720 724 728+ 732             exactly; W = 488, 728: the first width with a
                                                                `fast` wave in strip 1, in strips 1 and 2
  G3     215..240 x 12 and x 244 (217x244+, 229x244+)     3, 5  one segment (215, 216), then seg_rows 109..120:
                                                                every ya % 12 and every H % 12
  G3     432 433+ 434 648 649 x 12                        3, 5  2, 3, 3, 3, 4 segments
  G4     229x488+, 433x732+                               5, 3  `fast` waves across a segment seam
  G5     25x488, 229x492                                  3     bgr at 16-byte alignment + 1, 2, 3 and classes
                                                                at + 1: byte loads / stores at W % 4 == 0

Images of a batch, in this order (n = 5 repeats the first two with another seed): ``blocks``
(4 x 4 plateaus of level * step + 60, level 0..5, a step per block in 8..29: low contrast,
magnitudes on both thresholds and NMS ties in every direction), ``sat`` (3 x 3 blocks of 0 or
255: the largest magnitudes) and uniform random bytes (the synthetic UI image from 32 x 32).
"""
from __future__ import annotations

import functools

import numpy as np

from low_level_feature_extraction_amd import synth

STRIP_W, SEG, HALO = 240, 216, 8  # stencil_stream.hip: kStripW, LLFE_ST_SEG, kHalo


def geometry(h, w):
    """(strips, segs, seg_rows) as stream_geometry computes them."""
    strips = (w + STRIP_W - 1) // STRIP_W
    segs = max(1, (h + SEG - 1) // SEG)
    seg_rows = (h + segs - 1) // segs
    return strips, (h + seg_rows - 1) // seg_rows, seg_rows


def fast_strips(w):
    """Strips whose 256-column window lies inside the image (12-byte loads when W % 4 == 0)."""
    return [s for s in range(geometry(1, w)[0]) if s * STRIP_W - HALO >= 0 and s * STRIP_W - HALO + 256 <= w]


G1 = tuple((h, w) for h in (1, 2, 3, 4, 5, 6, 7, 13) for w in range(1, 13))
G2 = tuple((13, w) for w in (236, 239, 240, 241, 243, 244, 248, 252, 476, 480, 481, 484, 488, 492, 720, 724, 728, 732))
G3 = tuple((h, w) for w in (12, 244) for h in range(215, 241)) + tuple((h, 12) for h in (432, 433, 434, 648, 649))
G4 = ((229, 488), (433, 732))
G5 = ((25, 488), (229, 492))
PROCESS = frozenset([(13, 241), (13, 244), (13, 480), (13, 488), (13, 728), (217, 244), (229, 244), (433, 12)]
                    + list(G4))
FIVE = frozenset([(13, 241), (13, 481), (229, 12), (433, 12), (229, 488)])  # n * strips * segs = 10, 15, 10, 15, 30
SHAPES = G1 + G2 + G3 + G4


def blocks(h, w, seed):
    rng = np.random.default_rng([1, seed, h, w])
    bh, bw = (h + 3) // 4, (w + 3) // 4
    v = rng.integers(0, 6, (bh, bw)) * rng.integers(8, 30, (bh, bw)) + 60
    v = np.kron(v, np.ones((4, 4), np.int64))[:h, :w].astype(np.uint8)
    return np.ascontiguousarray(np.repeat(v[:, :, None], 3, 2))


def sat(h, w, seed):
    rng = np.random.default_rng([2, seed, h, w])
    v = rng.integers(0, 2, ((h + 2) // 3, (w + 2) // 3)) * 255
    v = np.kron(v, np.ones((3, 3), np.int64))[:h, :w].astype(np.uint8)
    return np.ascontiguousarray(np.repeat(v[:, :, None], 3, 2))


def rand(h, w, seed):
    if h >= 32 and w >= 32:
        return synth.synth_numpy(seed, h, w, seed=17)
    return np.random.default_rng([3, seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def images(h, w):
    x = [blocks(h, w, 0), sat(h, w, 0), rand(h, w, 0)]
    if (h, w) in FIVE:
        x += [blocks(h, w, 1), sat(h, w, 1)]
    x = np.stack(x)
    x.setflags(write=False)
    return x


def _orc():
    from oracle import oracle

    oracle.lib()
    return oracle


@functools.lru_cache(maxsize=None)
def expected(h, w):
    """(classes n x h x w, [(shadow_sum, shadow_count)], masks n x h x w) of the oracle."""
    O = _orc()
    x = images(h, w)
    cls = np.stack([O.canny_nms(O.blur5(O.bgr2gray(i))) for i in x])
    shadow = [O.shadow_stats(i) for i in x]
    mask = np.stack([O.shape_mask(i) for i in x])
    cls.setflags(write=False)
    mask.setflags(write=False)
    return cls, shadow, mask


def tie_counts(img):
    """The pixels of one image on each threshold and NMS tie, from the oracle's stages."""
    O = _orc()
    blur = O.blur5(O.bgr2gray(img))
    dx, dy = (a.astype(np.int64) for a in O.sobel3(blur))
    m = np.abs(dx) + np.abs(dy)
    p = np.pad(m, 1)  # no magnitude outside the image
    h, w = m.shape
    nb = {(a, b): p[1 + a:1 + a + h, 1 + b:1 + b + w] for a in (-1, 0, 1) for b in (-1, 0, 1)}
    ax, ay = np.abs(dx), np.abs(dy) << 15
    tg22 = ax * 13573
    cand = m > 50
    hor = cand & (ay < tg22)
    ver = cand & ~hor & (ay > tg22 + (ax << 16))
    dia = cand & ~hor & ~ver
    neg = (dx ^ dy) < 0  # the diagonal through (-1, +1) and (+1, -1)
    d = np.asarray(O.gauss_float_mean(blur), np.int64) - blur
    return {
        "odd": int((m % 2).sum()), "max": int(m.max()),
        "m50": int((m == 50).sum()), "m52": int((m == 52).sum()), "m150": int((m == 150).sum()),
        "m152": int((m == 152).sum()),
        "left": int((hor & (m == nb[0, -1])).sum()), "right": int((hor & (m == nb[0, 1])).sum()),
        "up": int((ver & (m == nb[-1, 0])).sum()), "down": int((ver & (m == nb[1, 0])).sum()),
        "diag_ul": int((dia & ~neg & (m == nb[-1, -1])).sum()), "diag_dr": int((dia & ~neg & (m == nb[1, 1])).sum()),
        "diag_ur": int((dia & neg & (m == nb[-1, 1])).sum()), "diag_dl": int((dia & neg & (m == nb[1, -1])).sum()),
        "shadow1": int((d == 1).sum()), "shadow2": int((d == 2).sum()),
    }
