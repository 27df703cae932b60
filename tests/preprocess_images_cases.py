"""Case tables for llfe_preprocess_images / llfe_resize_cv_images (cvresize_images.hip): the
resize of validate_and_preprocess_image over a batch of images of any sizes.

tests/test_preprocess_images_inputs.py checks on the CPU that the tables reach the plans they
claim (resize_cases.cv_plan, the restatement of cv_resize_plan) and that a second NumPy statement
of cv2.resize agrees with the oracle on them; tests/test_gpu_preprocess_images.py runs the device
on the same cases, byte for byte.  Images come from resize_cases.images(h, w, 3) (uniform random,
random 0 / 255, one-pixel checkerboard) and expected values from the oracle's cv_resize; both are
computed once and shared: callers must not modify them.

RULE_CASES: per preprocessing mode, (h, w) -> (oh, ow) under the rule and what cv2.resize makes of
it.  SEAM sizes are derived from the kernels' tiling (seam_cases): results of three full tiles and
a partial one in each axis at non-integer scales 1.3 and 2.016 (AREA), integer scales 2 and 3
(AREA_FAST), LINEAR and LANCZOS4 at the same four scales, and four images whose scale of 31 and more in one axis forces
the smallest tile height or the arm that reads global memory.  LARGE_SIZES: three photo sizes
under "auto" (device test only: the NumPy statement walks AREA_FAST pixel by pixel).
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import resize_cases as RC

MAX_DIM = {"auto": (2000, "area"), "high_quality": (4000, "lanczos4"), "performance": (1000, "linear")}
CODE = {"linear": 1, "area": 3, "lanczos4": 4}


def rule(h, w, mode):
    """validate_and_preprocess_image's size rule: (oh, ow, interpolation name) or None."""
    if mode not in MAX_DIM:
        return None
    max_dim, interp = MAX_DIM[mode]
    if max(h, w) <= max_dim:
        return None
    scale = max_dim / max(h, w)
    return int(h * scale), int(w * scale), interp


class RuleCase(NamedTuple):
    mode: str
    h: int
    w: int
    oh: int
    ow: int
    kind: str  # COPY / AREA_FAST / AREA / GENERIC as cv2.resize classifies it
    facts: dict  # fields of resize_cases.CvPlan the case stands for

    @property
    def id(self):
        return f"{self.mode}-{self.h}x{self.w}-to-{self.oh}x{self.ow}"

    @property
    def interp(self):
        return MAX_DIM[self.mode][1]

    @property
    def resized(self):
        return (self.oh, self.ow) != (self.h, self.w)


RULE_CASES = (
    RuleCase("auto", 6, 4000, 3, 2000, "AREA_FAST", {"fx": 2, "fy": 2}),
    RuleCase("auto", 6000, 9, 2000, 3, "AREA_FAST", {"fx": 3, "fy": 3}),
    RuleCase("auto", 7, 2001, 6, 2000, "AREA", {"fx": 2001 / 2000, "fy": 7 / 6}),
    RuleCase("auto", 9, 4032, 4, 2000, "AREA", {"fx": 2.016, "fy": 2.25}),
    RuleCase("auto", 2001, 5, 2000, 4, "AREA", {}),
    RuleCase("auto", 13, 3001, 8, 1999, "AREA", {}),
    RuleCase("auto", 2000, 2000, 2000, 2000, "COPY", {}),
    RuleCase("performance", 10, 2000, 5, 1000, "AREA_FAST", {"interp": "area", "fx": 2, "fy": 2}),
    RuleCase("performance", 7, 1001, 6, 1000, "GENERIC", {"ks": 2, "x_vec": 2992, "tail": 8}),
    RuleCase("performance", 1300, 11, 1000, 8, "GENERIC", {"ks": 2, "xmax": 8, "x_vec": 16, "tail": 8}),
    RuleCase("high_quality", 9, 4001, 8, 4000, "GENERIC", {"ks": 8, "xmin": 3, "xmax": 3997}),
    RuleCase("high_quality", 5000, 12, 4000, 9, "GENERIC", {"ks": 8, "xmin": 3, "xmax": 6}),
)
MODES = ("auto", "performance", "high_quality")
ZERO_SIDE = ("auto", 1, 2001)  # the rule gives 0 x 2000: cv2.resize raises, the call refuses


def rule_cases(mode):
    return [c for c in RULE_CASES if c.mode == mode]


class SeamCase(NamedTuple):
    name: str
    h: int
    w: int
    oh: int
    ow: int
    interp: str
    kind: str

    @property
    def id(self):
        return f"{self.name}-{self.interp}-{self.h}x{self.w}-to-{self.oh}x{self.ow}"


N_SEAM = 12  # the first N_SEAM of seam_cases stand on the tile seams


def seam_cases(tile_w, tile_h):
    """Results of 3 full tiles and a partial one per axis (the sources stay below 700 x 900), then
    the images whose scale forces the smallest tiles or the global-memory arm."""
    oh, ow = 3 * tile_h + 5, 3 * tile_w + 11
    out = []
    for name, s, interp, kind in (("s1.3", 1.3, "area", "AREA"), ("s2.016", 2.016, "area", "AREA"),
                                  ("s2", 2, "area", "AREA_FAST"), ("s3", 3, "area", "AREA_FAST"),
                                  ("s1.3", 1.3, "linear", "GENERIC"), ("s2.016", 2.016, "linear", "GENERIC"),
                                  ("s2", 2, "linear", "AREA_FAST"),  # LINEAR at exactly 2 x 2 runs as AREA
                                  ("s3", 3, "linear", "GENERIC"),
                                  ("s1.3", 1.3, "lanczos4", "GENERIC"), ("s2.016", 2.016, "lanczos4", "GENERIC"),
                                  ("s2", 2, "lanczos4", "GENERIC"), ("s3", 3, "lanczos4", "GENERIC")):
        out.append(SeamCase(name, round(oh * s), round(ow * s), oh, ow, interp, kind))
    assert len(out) == N_SEAM
    out += [SeamCase("fy31", 3100, 40, 100, 40, "area", "AREA_FAST"),  # the issue's example: exactly 31 x 1
            SeamCase("sy31.1", 3110, 40, 100, 40, "area", "AREA"),  # one output row per tile
            SeamCase("sx31.1", 40, 3110, 40, 100, "area", "AREA"),  # the x table slice exceeds LDS: global arm
            SeamCase("fx100", 40, 10000, 40, 100, "area", "AREA_FAST")]  # a tile's source row exceeds LDS
    return out


LARGE_SIZES = ((3024, 4032), (2160, 3840), (3000, 4000))  # the last is AREA_FAST 2 x 2


def image(h, w, k=0):
    """One of resize_cases.images(h, w, 3): k picks rand / sat / checker (read-only)."""
    return RC.images(h, w, 3)[k % 3]


@functools.lru_cache(maxsize=None)
def expected(h, w, oh, ow, interp, k=0):
    """The oracle's cv_resize of image(h, w, k) (read-only); the image itself when the size stays."""
    x = image(h, w, k)
    if (oh, ow) == (h, w):
        return x
    out = RC._orc().cv_resize(x, ow, oh, interp)
    out.setflags(write=False)
    return out


def rule_batch(mode):
    """(images, expected) of a mode's cases; image k of the batch is of kind k % 3."""
    cases = rule_cases(mode)
    return ([image(c.h, c.w, k) for k, c in enumerate(cases)],
            [expected(c.h, c.w, c.oh, c.ow, c.interp, k) for k, c in enumerate(cases)])


def seam_batch(tile_w, tile_h):
    cases = seam_cases(tile_w, tile_h)
    return (cases, [image(c.h, c.w, k) for k, c in enumerate(cases)],
            [expected(c.h, c.w, c.oh, c.ow, c.interp, k) for k, c in enumerate(cases)])


def stage_cases():
    """Every three-channel area / linear / lanczos4 case of resize_cases.CV_CASES."""
    return [c for c in RC.CV_CASES if c.cn == 3 and c.interp in ("area", "linear", "lanczos4")]


@functools.lru_cache(maxsize=None)
def large_batch():
    imgs = [np.random.default_rng([21, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in LARGE_SIZES]
    exp = []
    for x in imgs:
        x.setflags(write=False)
        oh, ow, interp = rule(x.shape[0], x.shape[1], "auto")
        e = RC._orc().cv_resize(x, ow, oh, interp)
        e.setflags(write=False)
        exp.append(e)
    return imgs, exp
