"""Shared by tests/test_jpeg_orient_host.py and tests/test_gpu_jpeg_orient.py: JPEGs that carry an
EXIF orientation, and the orientation table of csrc/jpeg_orient.h restated with NumPy index
arrays, one line per row of the table."""
import io

import numpy as np
from PIL import Image

ORIENTATIONS = tuple(range(1, 9))


def jpeg(arr, orientation=None, **kw):
    """``arr`` (h x w x 3 RGB, h x w grey, or h x w x 4 CMYK) as a JPEG; ``orientation``: the value
    of EXIF tag 0x0112 (None: no EXIF at all).  The coded raster is ``arr`` in every case."""
    b = io.BytesIO()
    if orientation is not None:
        ex = Image.Exif()
        ex[0x0112] = orientation
        kw["exif"] = ex.tobytes()
    Image.fromarray(arr, "CMYK" if arr.ndim == 3 and arr.shape[2] == 4 else None).save(b, "JPEG", **kw)
    return b.getvalue()


def reindex(s, o):
    """The result O of orientation ``o`` for the coded raster ``s`` (h x w [x c])."""
    h, w = s.shape[:2]
    y, x = np.indices((w, h) if o >= 5 else (h, w))
    return {1: lambda: s[y, x],
            2: lambda: s[y, w - 1 - x],
            3: lambda: s[h - 1 - y, w - 1 - x],
            4: lambda: s[h - 1 - y, x],
            5: lambda: s[x, y],
            6: lambda: s[h - 1 - x, y],
            7: lambda: s[h - 1 - x, w - 1 - y],
            8: lambda: s[x, w - 1 - y]}[o]()


def pixels(h, w, seed):
    """h x w x 3 noise: every pixel differs from its neighbours, so a misplaced one shows."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
