"""Directed cases for llfe_thumbnail_pil_images (thumb_images.hip): thumbnails of a batch whose
images each have their own size.

Each table is one batch for one box.  tests/test_thumb_images_inputs.py checks on the CPU,
through resize_cases.thumb_plan and pil_plan, that the tables reach the branches the notes
claim; tests/test_gpu_thumb_images.py runs each table through one device call, byte-identical
to Pillow's own Image.thumbnail.  Images and expected values are computed once and shared
(``functools.lru_cache``): callers must not modify them.

Box (50, 50), sources h x w:
  37 x 401   -> 5 x 50, factors (4, 3), remainders (1, 1)
  20 x 30    fits: copied
  50 x 50    fits exactly: copied
  50 x 70    -> 36 x 50, no pre-pass
  33 x 100   -> 17 x 50, no pre-pass: scale exactly 2.0 in x
  300 x 210  -> 50 x 35, factors (3, 3), no remainder
  301 x 212  -> 50 x 35, factors (3, 3), remainders (2, 1)
  9 x 1000   -> 1 x 50, factors (10, 4)
  1000 x 9   -> 50 x 1, factors (4, 10)
  1 x 120    -> 1 x 50: the horizontal pass only
  120 x 1    -> 50 x 1: the vertical pass only
  51 x 51    -> 50 x 50, scale 1.02
  200 x 199  -> 50 x 50, factors (1, 2): residual scale 3.98 in x, ksize 25, the kernel's bound

Box (300, 200):
  431 x 647   -> 200 x 300, no pre-pass, scale 2.16
  880 x 1320  -> 200 x 300, factors (2, 2)
  883 x 1321  -> 200 x 299, factors (2, 2), remainders (1, 1)
  200 x 300   fits: copied
  647 x 431   -> 200 x 133, no pre-pass, scale 3.24
  201 x 300   -> 200 x 299

Image contents alternate between resize_cases.images' "rand" and "sat" (random 0 / 255, which
reaches both clamps of clip8).
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import resize_cases as RC


class Case(NamedTuple):
    h: int
    w: int
    oh: int  # the result Pillow gives
    ow: int
    factors: tuple | None  # (fx, fy) of the pre-pass; None: no pre-pass
    remainders: tuple = (0, 0)  # (w % fx, h % fy)
    fits: bool = False

    @property
    def id(self):
        return f"{self.h}x{self.w}"


BOX_SMALL = (50, 50)  # (max_w, max_h)
CASES_SMALL = (
    Case(37, 401, 5, 50, (4, 3), (1, 1)),
    Case(20, 30, 20, 30, None, fits=True),
    Case(50, 50, 50, 50, None, fits=True),
    Case(50, 70, 36, 50, None),
    Case(33, 100, 17, 50, None),
    Case(300, 210, 50, 35, (3, 3)),
    Case(301, 212, 50, 35, (3, 3), (2, 1)),
    Case(9, 1000, 1, 50, (10, 4), (0, 1)),
    Case(1000, 9, 50, 1, (4, 10), (1, 0)),
    Case(1, 120, 1, 50, None),
    Case(120, 1, 50, 1, None),
    Case(51, 51, 50, 50, None),
    Case(200, 199, 50, 50, (1, 2)),
)
BOX_LARGE = (300, 200)
CASES_LARGE = (
    Case(431, 647, 200, 300, None),
    Case(880, 1320, 200, 300, (2, 2)),
    Case(883, 1321, 200, 299, (2, 2), (1, 1)),
    Case(200, 300, 200, 300, None, fits=True),
    Case(647, 431, 200, 133, None),
    Case(201, 300, 200, 299, None),
)
TABLES = {"box50": (BOX_SMALL, CASES_SMALL), "box300x200": (BOX_LARGE, CASES_LARGE)}
KSIZE_BOUND_CASE = (200, 199)  # the source whose horizontal filter has the widest ksize there is
LARGE_SIZES = ((2160, 3840), (3024, 4032), (5000, 2400))  # at the default box (1920, 1080)
DEFAULT_BOX = (1920, 1080)


def image(h, w, k):
    """The k-th image of a table: "rand" for even k, "sat" for odd k; seed k keeps three images of
    one size apart."""
    return RC.images(h, w, 3, seed=k)[k & 1]


def batch(name):
    """The sources of a table, in its order (read-only arrays)."""
    return [image(c.h, c.w, k) for k, c in enumerate(TABLES[name][1])]


def pil_thumbnail(img, box):
    """Pillow's own Image.thumbnail(box, LANCZOS) of an H x W x 3 array."""
    from PIL import Image

    im = Image.fromarray(np.asarray(img))
    im.thumbnail(box, Image.Resampling.LANCZOS)
    out = np.array(im)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    box = TABLES[name][0]
    return tuple(pil_thumbnail(x, box) for x in batch(name))


@functools.lru_cache(maxsize=None)
def large_batch():
    """(sources, Pillow's thumbnails) of LARGE_SIZES at the default box."""
    src = tuple(RC.thumb_image(h, w, 3, 40 + k) for k, (h, w) in enumerate(LARGE_SIZES))
    return src, tuple(pil_thumbnail(x, DEFAULT_BOX) for x in src)
