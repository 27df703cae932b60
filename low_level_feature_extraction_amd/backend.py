"""Device-side entry points over the C ABI (one context per GPU per host thread).

``Backend`` owns an ``llfe_ctx`` for one device and exposes the batch pipeline and the
stage functions with numpy / torch arguments.  Device memory for host inputs is
handled by the library itself (``on_device = 0``); torch tensors already on the GPU are
passed by pointer together with torch's current HIP stream, so no copy is made.

Nothing in this module computes features on the CPU: a missing ``libllfe.so`` or a
missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L

FEATURE_BITS = {"colors": L.FEATURE_COLORS, "shapes": L.FEATURE_SHAPES, "shadows": L.FEATURE_SHADOWS,
                "fonts": L.FEATURE_FONTS}


SHADOW_LEVELS = ("Low", "Moderate", "High")  # llfe_image_result.shadow_level 0 / 1 / 2


def feature_mask(features) -> int:
    m = 0
    for f in features:
        f = getattr(f, "value", f)
        if f not in FEATURE_BITS:
            raise ValueError(f"unknown feature {f!r}")
        m |= FEATURE_BITS[f]
    return m


@dataclass
class ImageFeatures:
    """Per-image output of the batched hot path (pre-assembly)."""

    centers_rgb: np.ndarray  # (K, 3) uint8, k-means order
    counts: np.ndarray       # (K,) unique colours per centre
    n_unique: int
    compactness: float
    shadow_sum: int
    shadow_count: int
    shapes: list = field(default_factory=list)
    n_contours: int = 0
    width: int = 0
    height: int = 0
    # made in C on the host half of collect / process (llfe_image_result): extract_colors'
    # palette (primary, background, [3 accents]) and analyze_shadow_level's level
    palette: tuple | None = None
    shadow_level: str | None = None
    # "fonts": the image's llfe_font_result as font_detect's dict (n_contours, n_regions, x, y,
    # width, height, gray_sum)
    font: dict | None = None


def _torch():
    import torch

    return torch


def _is_torch(x) -> bool:
    try:
        import torch
    except ImportError:  # pragma: no cover
        return False
    return isinstance(x, torch.Tensor)


def _default_device(device: int | None = None) -> int:
    if device is None:
        device = int(os.environ.get("LLFE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    return device


_DESC_DTYPE = None  # np.dtype(L.LlfeImageDesc), made at the first use


def _image_descs(images, device: int):
    """The llfe_image_desc records of a list of H x W x 3 uint8 images, numpy arrays (host) or
    torch tensors (host or the GPU ``device``), for process_images and submit_images:
    -> (numpy structured array with data / height / width / row_stride / on_device filled, keep-alive
    list, heights, widths, the first device tensor or None).  An image is read in place when its
    pixels are packed and its rows do not overlap (rows may be strided), and otherwise gets one
    packed copy.  A device tensor on another GPU than ``device`` raises ValueError: its pointer
    means nothing to this context."""
    global _DESC_DTYPE
    if _DESC_DTYPE is None:
        _DESC_DTYPE = np.dtype(L.LlfeImageDesc)
    keep, ptr, hh, ww, st, dev = [], [], [], [], [], []
    u8 = first = None
    for i, im in enumerate(images):
        if _is_torch(im):
            # (few attribute calls per image: at serving rates this loop holds the GIL once per
            # request; a contiguous tensor needs no look at its strides)
            if u8 is None:
                u8 = _torch().uint8
            shp = im.shape
            if len(shp) != 3 or shp[2] != 3 or im.dtype != u8:
                raise ValueError(f"image {i}: expected H x W x 3 uint8, got {tuple(shp)} {im.dtype}")
            t, stride = im, 3 * shp[1]
            if not t.is_contiguous():
                if t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < stride:
                    t = t.contiguous()  # pixels not packed, or rows overlap (stride 0): one copy
                else:
                    stride = t.stride(0)
            on_dev = 1 if t.is_cuda else 0
            if on_dev:
                if t.device.index != device:
                    raise ValueError(f"image {i}: tensor on cuda:{t.device.index}, context on cuda:{device}")
                if first is None:
                    first = t
            ptr.append(t.data_ptr())
        else:
            t = np.asarray(im)
            if t.dtype != np.uint8 or t.ndim != 3 or t.shape[2] != 3:
                raise ValueError(f"image {i}: expected H x W x 3 uint8, got {t.shape} {t.dtype}")
            shp = t.shape
            if t.strides[2] != 1 or t.strides[1] != 3 or t.strides[0] < 3 * shp[1]:
                t = np.ascontiguousarray(t)
            ptr.append(t.ctypes.data)
            stride, on_dev = t.strides[0], 0
        dev.append(on_dev)
        st.append(stride)
        hh.append(shp[0])
        ww.append(shp[1])
        keep.append(t)
    descs = np.zeros(len(keep), _DESC_DTYPE)
    descs["data"], descs["height"], descs["width"] = ptr, hh, ww
    descs["row_stride"], descs["on_device"] = st, dev
    return descs, keep, hh, ww, first


def _dev_u8_2d(name: str, t, shape: str = "2-d"):
    if not (_is_torch(t) and t.is_cuda and t.dtype == _torch().uint8 and t.dim() == 2 and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {shape} uint8 device tensor")


def _shape_dict(s) -> dict:
    return {"type": L.SHAPE_TYPES[s.type], "x": int(s.x), "y": int(s.y), "width": int(s.width),
            "height": int(s.height), "border_radius": float(s.border_radius), "area": float(s.area)}


def _font_dict(r) -> dict:
    return {k: int(getattr(r, k)) for k in _FONT_FIELDS}


def font_bits_tiling(h: int, w: int):
    """(strip width, segment height) of k_font_bits for an h x w image (llfe_font_bits_tiling)."""
    sw, sh = C.c_int32(0), C.c_int32(0)
    if L.lib().llfe_font_bits_tiling(int(h), int(w), C.byref(sw), C.byref(sh)) < 0:
        raise ValueError(f"font_bits_tiling: invalid {h}x{w}")
    return sw.value, sh.value


def thumbnail_images_tiling():
    """(tile width, largest tile height, LDS rows, largest ksize) of k_thumb_lanczos
    (llfe_thumbnail_images_tiling)."""
    v = [C.c_int32(0) for _ in range(4)]
    if L.lib().llfe_thumbnail_images_tiling(*[C.byref(x) for x in v]) < 0:  # pragma: no cover
        raise ValueError("thumbnail_images_tiling")
    return tuple(x.value for x in v)


def jpeg_images_tiling(sampling: int):
    """(tile width, tile height) of k_jpeg_images for a sampling class (llfe_jpeg_images_tiling)."""
    tw, th = C.c_int32(0), C.c_int32(0)
    if L.lib().llfe_jpeg_images_tiling(int(sampling), C.byref(tw), C.byref(th)) < 0:
        raise ValueError(f"jpeg_images_tiling: unknown sampling class {sampling}")
    return tw.value, th.value


COLOR_ROUTES = {"grouped": 0, "one_pass": L.IMAGES_COLORS_ONE_PASS}


def colors_flags(colors: str) -> int:
    """The llfe_process_images_flags bits of process_images' ``colors`` option."""
    try:
        return COLOR_ROUTES[colors]
    except (KeyError, TypeError):
        raise ValueError(f"colors must be one of {sorted(COLOR_ROUTES)}, got {colors!r}") from None


SHAPE_ROUTES = {"grouped": 0, "one_pass": L.IMAGES_SHAPES_ONE_PASS}


def shapes_flags(shapes: str) -> int:
    """The shapes_flags word of llfe_process_images_routes for process_images' ``shapes`` option."""
    try:
        return SHAPE_ROUTES[shapes]
    except (KeyError, TypeError):
        raise ValueError(f"shapes must be one of {sorted(SHAPE_ROUTES)}, got {shapes!r}") from None


def _images_layout(fn: str, types, images, preprocessing: str, device: int):
    """(per-image records, work table, passes) of a host-only pass planner as lists of dicts."""
    descs, keep, _, _, _ = _image_descs(images, device)
    n = len(keep)
    mode = PRE_MODES.get(preprocessing, 0)
    nw, npass = C.c_int64(0), C.c_int32(0)
    plan = getattr(L.lib(), fn)
    rc = plan(descs.ctypes.data, n, mode, None, None, 0, C.byref(nw), None, 0, C.byref(npass))
    if rc < 0:
        raise L.LlfeError(rc, "invalid image list")
    recs = (types[0] * max(n, 1))()
    work = (types[1] * max(nw.value, 1))()
    passes = (types[2] * max(npass.value, 1))()
    rc = plan(descs.ctypes.data, n, mode, recs, work, nw.value, C.byref(nw), passes, npass.value, C.byref(npass))
    if rc < 0:  # pragma: no cover
        raise L.LlfeError(rc, "invalid image list")

    def dicts(arr, m):
        return [{f.rstrip("_") if f == "pass_" else f: int(getattr(r, f)) for f, _ in r._fields_ if f != "pad_"}
                for r in arr[:m]]

    return dicts(recs, n), dicts(work, nw.value), dicts(passes, npass.value)


def colors_images_layout(images, preprocessing: str = "none", device: int = 0):
    """The colour passes process_images(..., colors="one_pass") runs (llfe_colors_images_layout,
    host only): -> (per-image records, work table, passes) as lists of dicts."""
    return _images_layout("llfe_colors_images_layout", (L.LlfeColorImage, L.LlfeColorWork, L.LlfeColorPass), images,
                          preprocessing, device)


def shapes_images_layout(images, preprocessing: str = "none", device: int = 0):
    """The passes process_images(..., shapes="one_pass") runs (llfe_shapes_images_layout, host
    only): -> (per-image records, work table, passes) as lists of dicts."""
    return _images_layout("llfe_shapes_images_layout", (L.LlfeShapeImage, L.LlfeShapeWork, L.LlfeShapePass), images,
                          preprocessing, device)


def thumbnail_images_layout(images, max_w=1920, max_h=1080, device: int = 0):
    """Where llfe_thumbnail_pil_images puts each result: -> (list of (offset, height, width,
    resized), bytes the packed destination must hold).  Host only."""
    descs, keep, _, _, _ = _image_descs(images, device)
    outs = (L.LlfeThumbOut * max(len(keep), 1))()
    total = C.c_int64(0)
    rc = L.lib().llfe_thumbnail_images_layout(descs.ctypes.data, len(keep), int(max_w), int(max_h), outs,
                                              C.byref(total))
    if rc < 0:
        raise L.LlfeError(rc, "invalid thumbnail batch")
    return [(int(o.offset), int(o.height), int(o.width), int(o.resized)) for o in outs[:len(keep)]], int(total.value)


def resize_cv_images_tiling():
    """(tile width, largest tile height, LDS rows) of the k_cv_images_* kernels
    (llfe_resize_cv_images_tiling)."""
    v = [C.c_int32(0) for _ in range(3)]
    if L.lib().llfe_resize_cv_images_tiling(*[C.byref(x) for x in v]) < 0:  # pragma: no cover
        raise ValueError("resize_cv_images_tiling")
    return tuple(x.value for x in v)


def _pre_mode(preprocessing: str) -> int:
    try:
        return PRE_MODES[preprocessing]
    except (KeyError, TypeError):
        raise ValueError(f"preprocessing must be one of {sorted(PRE_MODES)}, got {preprocessing!r}") from None


def _resize_outs(outs, n):
    return [(int(o.offset), int(o.height), int(o.width), int(o.interpolation), int(o.resized)) for o in outs[:n]]


def preprocess_images_layout(images, preprocessing: str = "auto", device: int = 0):
    """Where llfe_preprocess_images puts each result: -> (list of (offset, height, width,
    interpolation code, resized), bytes the packed destination must hold).  Host only."""
    mode = _pre_mode(preprocessing)
    descs, keep, _, _, _ = _image_descs(images, device)
    outs = (L.LlfeResizeOut * max(len(keep), 1))()
    total = C.c_int64(0)
    rc = L.lib().llfe_preprocess_images_layout(descs.ctypes.data, len(keep), mode, outs, C.byref(total))
    if rc < 0:
        raise L.LlfeError(rc, "invalid preprocessing batch")
    return _resize_outs(outs, len(keep)), int(total.value)


PREPROCESS_ROUTES = ("per_image", "one_pass")


def preprocess_route(preprocess: str) -> str:
    """process_images' ``preprocess`` option, checked."""
    if preprocess not in PREPROCESS_ROUTES:
        raise ValueError(f"preprocess must be one of {sorted(PREPROCESS_ROUTES)}, got {preprocess!r}")
    return preprocess


def text_size(h: int, w: int):
    """Output (height, width) of TextExtractor.preprocess_image (llfe_text_size)."""
    oh, ow = C.c_int32(0), C.c_int32(0)
    if L.lib().llfe_text_size(int(h), int(w), C.byref(oh), C.byref(ow)) < 0:
        raise ValueError(f"text_size: invalid {h}x{w}")
    return oh.value, ow.value


class Backend:
    _instances: dict = {}
    _ilock = threading.Lock()

    def __init__(self, device: int | None = None):
        self.device = device = _default_device(device)
        # PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so) beside the
        # /opt/rocm one libllfe links: torch's must initialise first, or its later
        # lazy init finds "no HIP GPUs" once libllfe holds the device
        try:
            import torch

            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:  # pragma: no cover
            pass
        self._lib = L.lib()
        ctx = C.c_void_p()
        rc = self._lib.llfe_init(device, C.byref(ctx))
        if rc != L.LLFE_OK:
            raise L.LlfeError(rc, f"llfe_init(device={device}) failed (no HIP device available?)")
        self.ctx = ctx
        self._lock = threading.RLock()  # (re-entered by submit -> _call)
        self._inflight = {}  # ticket -> what collect needs; keeps the batch's inputs alive

    @classmethod
    def get(cls, device: int | None = None) -> "Backend":
        device = _default_device(device)
        key = (device, threading.get_ident())
        with cls._ilock:
            b = cls._instances.get(key)
            if b is None:
                b = cls._instances[key] = Backend(device)
            return b

    @classmethod
    def release(cls, backend: "Backend"):
        """Drop a thread's cached context (``get``) and free its device workspaces -- for a
        thread that is about to end, e.g. MicroBatcher's worker at close()."""
        with cls._ilock:
            for key, b in list(cls._instances.items()):
                if b is backend:
                    del cls._instances[key]
        backend.close()

    def close(self):
        if self.ctx:
            with self._lock:
                self._lib.llfe_destroy(self.ctx)
                self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ profiling
    def set_profiling(self, enable: bool):
        self._call("llfe_set_profiling", int(bool(enable)))

    def set_concurrency(self, enable: bool):
        """Colour path on a second stream beside shapes / shadows (default) or all kernels
        in order on one stream (isolated kernel timings)."""
        self._call("llfe_set_concurrency", int(bool(enable)))

    def set_contour_mode(self, mode: str):
        """"host" (default): findContours + shape geometry on the host pool while the GPU
        runs k-means; "gpu": on the GPU (contours_gpu.hip).  Identical results."""
        self._call("llfe_set_contour_mode", CONTOUR_MODES[mode])

    @property
    def inflight(self) -> int:
        """Batches ``submit`` keeps in flight (2 or 3; llfe_set_inflight)."""
        return self._call("llfe_get_inflight")

    @inflight.setter
    def inflight(self, depth: int):
        self._call("llfe_set_inflight", int(depth))

    def contour_mode(self) -> str:
        m = self._call("llfe_get_contour_mode")
        return {v: k for k, v in CONTOUR_MODES.items()}[m]

    def kernel_stats(self) -> dict:
        """{kernel: {"launches", "total_ms", "bytes"}} accumulated while profiling."""
        arr = (L.LlfeKernelStat * 64)()
        n = self._call("llfe_kernel_stats", arr, 64)
        return {arr[i].name.decode(): {"launches": int(arr[i].launches), "total_ms": float(arr[i].total_ms),
                                       "bytes": float(arr[i].bytes)} for i in range(min(n, 64))}

    def host_contour_stats(self, reset: bool = False) -> dict:
        """Host contour pool: busy wall ms, images traced and threads since the last reset."""
        ms, imgs, th = C.c_double(0), C.c_int64(0), C.c_int32(0)
        self._call("llfe_host_contour_stats", C.byref(ms), C.byref(imgs), C.byref(th), int(reset))
        return {"busy_ms": ms.value, "images": int(imgs.value), "threads": int(th.value)}

    # ------------------------------------------------------------------ helpers
    def _chk(self, rc):
        return L.check(self.ctx, rc)

    def _call(self, fn: str, *args):
        """self._lib.<fn>(ctx, *args) under the context lock, checked.  A ctx is not
        thread-safe (llfe.h): its scratch buffers are shared by every entry point, so a
        stage call from a request thread must not run beside a batch on the
        MicroBatcher thread."""
        with self._lock:
            return self._chk(getattr(self._lib, fn)(self.ctx, *args))

    def _stream(self, t=None):
        if t is not None and _is_torch(t) and t.is_cuda:
            torch = _torch()
            return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        return C.c_void_p(0)

    def _with_shapes(self, n, mask, ticket, call):
        """(results, shapes, font records) of one batch call for n images: ``call(results, shapes,
        capacity, needed)`` -> rc runs again with the shape array grown to ``needed`` when it
        returns LLFE_ERR_CAPACITY, and the font records of ``ticket`` (or L.LAST_CALL) are
        fetched under the same lock hold, so no other call comes between."""
        results = (L.LlfeImageResult * max(n, 1))()
        cap = max(64 * n, 64)
        needed = C.c_int64(0)
        with self._lock:
            while True:
                shapes = (L.LlfeShape * cap)()
                rc = call(results, shapes, cap, C.byref(needed))
                if rc == L.LLFE_ERR_CAPACITY and needed.value > cap:
                    cap = int(needed.value)
                    continue
                self._chk(rc)
                break
            return results, shapes, self._font_records(ticket, n, mask)

    @staticmethod
    def _batch_view(images):
        """-> (pointer, n, h, w, on_device, keepalive)"""
        if _is_torch(images):
            t = images
            if t.dtype != _torch().uint8 or t.dim() != 4 or t.shape[-1] != 3:
                raise ValueError(f"expected N x H x W x 3 uint8 tensor, got {tuple(t.shape)} {t.dtype}")
            t = t.contiguous()
            return t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], int(t.is_cuda), t
        a = np.ascontiguousarray(images, dtype=np.uint8)
        if a.ndim == 3:
            a = a[None]
        if a.ndim != 4 or a.shape[-1] != 3:
            raise ValueError(f"expected N x H x W x 3 uint8 array, got {a.shape}")
        return a.ctypes.data, a.shape[0], a.shape[1], a.shape[2], 0, a

    @staticmethod
    def _noise_view(noise, n, h, w):
        if noise is None:
            return None, 0, None
        if _is_torch(noise):
            t = noise.contiguous()
            if t.numel() != n * h * w * 3:
                raise ValueError("noise must hold N*H*W*3 int8 values")
            return t.data_ptr(), int(t.is_cuda), t
        a = np.ascontiguousarray(noise, dtype=np.int8)
        if a.size != n * h * w * 3:
            raise ValueError("noise must hold N*H*W*3 int8 values")
        return a.ctypes.data, 0, a

    # ------------------------------------------------------------------ hot path
    def process(self, images, features=("colors", "shapes", "shadows"), seed: int = 0, noise=None,
                index_base: int = 0, n_colors: int = 5) -> list:
        """Run the batched hot path. ``images``: N x H x W x 3 BGR uint8 (numpy host
        array or torch tensor, host or GPU).  Returns a list of ImageFeatures."""
        ptr, n, h, w, on_dev, keep = self._batch_view(images)
        nptr, n_on_dev, nkeep = self._noise_view(noise, n, h, w)
        mask = feature_mask(features)
        b = L.LlfeBatch(C.c_void_p(ptr), n, h, w, on_dev, C.c_void_p(nptr) if nptr else None, n_on_dev,
                        int(n_colors), index_base)
        stream = self._stream(keep)
        results, shapes, fonts = self._with_shapes(n, mask, L.LAST_CALL, lambda res, sh, cap, need: (
            self._lib.llfe_process_batch(self.ctx, C.byref(b), mask, C.c_uint64(seed & (2**64 - 1)), res, sh, cap,
                                         need, stream)))
        out = self._convert(results, shapes, n, mask, w, h, fonts)
        del keep, nkeep
        return out

    def process_images(self, images, features=("colors", "shapes", "shadows"), seed: int = 0, noise=None,
                       index_base: int = 0, n_colors: int = 5, preprocessing: str = "none",
                       colors: str = "grouped", shapes: str = "grouped", preprocess: str = "per_image") -> list:
        """Ragged batch through llfe_process_images: ``images`` is a list of H x W x 3 BGR
        uint8 images of any sizes -- numpy arrays (host) or torch tensors (host or GPU;
        rows may be strided, pixels must be packed) -- with validate_and_preprocess_image's
        resize rule (``preprocessing``: none / auto / high_quality / performance; other
        names do not resize, as in utils.py:116-143) applied on the GPU first.  Image i
        keeps global index index_base + i.  ``noise``: one parity-noise array per image of
        its preprocessed size, or None.  ``colors``: "grouped" runs the colours with the size
        groups; "one_pass" runs the colours of all images in one device pass whatever their
        sizes (LLFE_IMAGES_COLORS_ONE_PASS), with the same results.  ``shapes``: the same choice
        for shapes and shadows (LLFE_IMAGES_SHAPES_ONE_PASS: one stencil launch, one hysteresis,
        one mask copy and one fan-out over the host contour pool for the whole list; fonts stay
        grouped, and so do shapes and shadows while contours run on the GPU).  ``preprocess``:
        "per_image" resizes each image the rule resizes with a launch of its own inside the call;
        "one_pass" sends those images through one ``preprocess_images`` call first and proceeds
        with its device tensors in their places and no preprocessing, with the same results
        (the other images are passed through as they are).  Returns ImageFeatures in input
        order."""
        flags, sflags = colors_flags(colors), shapes_flags(shapes)
        n = len(images)
        mode = PRE_MODES.get(preprocessing, 0)
        descs, keep, hs, ws, first = _image_descs(images, self.device)
        if preprocess_route(preprocess) == "one_pass" and mode:
            idx = [i for i in range(n) if preprocess_size(ws[i], hs[i], preprocessing)]
            if idx:  # their records go through one call; its results take their places in `descs`
                res = self._preprocess_descs(np.ascontiguousarray(descs[idx]), first, mode)
                for i, t in zip(idx, res):
                    keep[i], hs[i], ws[i] = t, t.shape[0], t.shape[1]
                descs["data"][idx] = [t.data_ptr() for t in res]
                descs["height"][idx], descs["width"][idx] = [hs[i] for i in idx], [ws[i] for i in idx]
                descs["row_stride"][idx], descs["on_device"][idx] = [3 * ws[i] for i in idx], 1
                first = res[0] if first is None else first
            preprocessing, mode = "none", 0
        for i in range(n):
            plan = preprocess_size(ws[i], hs[i], preprocessing)
            if plan:
                ws[i], hs[i] = plan[0], plan[1]
        if noise is not None:
            nz = [self._noise_view(noise[i], 1, hs[i], ws[i]) for i in range(n)]
            descs["noise"], descs["noise_on_device"] = [v[0] or 0 for v in nz], [v[1] for v in nz]
            keep.append(nz)
        mask = feature_mask(features)
        stream = self._stream(first)
        results, shapes, fonts = self._with_shapes(n, mask, L.LAST_CALL, lambda res, sh, cap, need: (
            self._lib.llfe_process_images_routes(self.ctx, descs.ctypes.data, n, mask, mode, int(n_colors),
                                                 C.c_uint64(seed & (2**64 - 1)), index_base, res, sh, cap, need, stream,
                                                 flags, sflags)))
        out = self._convert(results, shapes, n, mask, ws, hs, fonts)
        del keep
        return out

    def _font_records(self, ticket: int, n: int, mask: int):
        """The font records of the call just made (llfe_font_records; the caller holds the
        context lock, so no other call comes between) as font_detect's dicts, or None
        without the fonts bit."""
        if not mask & L.FEATURE_FONTS:
            return None
        res = (L.LlfeFontResult * max(n, 1))()
        self._chk(self._lib.llfe_font_records(self.ctx, C.c_int64(ticket), res, n))
        F = np.ctypeslib.as_array(res)[:n]
        cols = [F[k].tolist() for k in _FONT_FIELDS]
        return [dict(zip(_FONT_FIELDS, v)) for v in zip(*cols)]

    @staticmethod
    def _convert(results, shapes, n, mask, w, h, fonts=None) -> list:
        # bulk conversion through numpy views of the ctypes arrays (per-field ctypes
        # access would cost ~20 us per image while the GPU waits for the next batch)
        R = np.ctypeslib.as_array(results)[:n]
        ncol = R["n_colors"].tolist()
        cen = R["centers_rgb"].copy()
        cnt = R["counts"].astype(np.int64)
        nu, comp = R["n_unique"].tolist(), R["compactness"].tolist()
        ssum, scnt = R["shadow_sum"].tolist(), R["shadow_count"].tolist()
        off, nsh, ncont = R["shape_offset"].tolist(), R["n_shapes"].tolist(), R["n_contours"].tolist()
        pal = [None] * n
        if mask & L.FEATURE_COLORS and n:
            def strs(f, shape):  # char[8] fields (numpy: 8 x S1) -> NUL-stripped bytes
                return np.ascontiguousarray(R[f]).view("S8").reshape(shape).tolist()

            pr, bg, ac = strs("primary", n), strs("background", n), strs("accent", (n, 3))
            pal = [(p.decode(), b.decode(), [a[0].decode(), a[1].decode(), a[2].decode()])
                   for p, b, a in zip(pr, bg, ac)]
        lv = [None] * n
        if mask & L.FEATURE_SHADOWS and n:
            lv = [SHADOW_LEVELS[v] for v in R["shadow_level"].tolist()]
        recs = []
        if mask & L.FEATURE_SHAPES and n:
            tot = max(o + c for o, c in zip(off, nsh))
            S = np.ctypeslib.as_array(shapes)[:tot]
            names = L.SHAPE_TYPES
            recs = [{"type": names[t], "x": x, "y": y, "width": ww, "height": hh, "border_radius": br, "area": ar}
                    for t, x, y, ww, hh, br, ar in zip(S["type"].tolist(), S["x"].tolist(), S["y"].tolist(),
                                                       S["width"].tolist(), S["height"].tolist(),
                                                       S["border_radius"].tolist(), S["area"].tolist())]
        ws = w if isinstance(w, list) else [w] * n
        hs = h if isinstance(h, list) else [h] * n
        out = [ImageFeatures(cen[i, :ncol[i]], cnt[i, :ncol[i]], nu[i], comp[i], ssum[i], scnt[i],
                             recs[off[i]:off[i] + nsh[i]] if recs else [], ncont[i], ws[i], hs[i], pal[i], lv[i],
                             fonts[i] if fonts else None)
               for i in range(n)]
        return out

    # ------------------------------------------------------------------ async batches
    def submit(self, images, features=("colors", "shapes", "shadows"), seed: int = 0, noise=None,
               index_base: int = 0, n_colors: int = 5) -> int:
        """Enqueue one batch (llfe_submit_batch) and return its ticket; at most
        ``inflight`` (default 2) in flight.  Results: ``collect(ticket)``, in submission order."""
        ptr, n, h, w, on_dev, keep = self._batch_view(images)
        nptr, n_on_dev, nkeep = self._noise_view(noise, n, h, w)
        mask = feature_mask(features)
        b = L.LlfeBatch(C.c_void_p(ptr), n, h, w, on_dev, C.c_void_p(nptr) if nptr else None, n_on_dev,
                        int(n_colors), index_base)
        ticket = C.c_int64(0)
        self._call("llfe_submit_batch", C.byref(b), mask, C.c_uint64(seed & (2**64 - 1)), self._stream(keep),
                   C.byref(ticket))
        self._inflight[ticket.value] = (n, h, w, mask, keep, nkeep, b)  # inputs stay alive
        return ticket.value

    def batch_capacity(self, h: int, w: int) -> int:
        """Images of h x w one ``submit`` / ``submit_images`` launch takes."""
        return L.check(self.ctx, self._lib.llfe_batch_capacity(int(h), int(w)))

    def submit_images(self, images, features=("colors", "shapes", "shadows"), seed: int = 0, indices=None,
                      n_colors: int = 5) -> int:
        """llfe_submit_images: n separately allocated H x W x 3 BGR uint8 images of one size
        (torch tensors on the device, or host arrays; rows may be strided, pixels packed),
        gathered into one launch, image i under global index ``indices[i]``.  Same ticket /
        ``collect`` / in-flight rules as ``submit``; the images must stay alive until then
        (the backend holds references)."""
        n = len(images)
        if n < 1:
            raise ValueError("submit_images needs at least one image")
        descs, keep, hh, ww, first = _image_descs(images, self.device)
        idx = np.ascontiguousarray(np.arange(n) if indices is None else indices, dtype=np.int64)
        if idx.shape != (n,):
            raise ValueError("indices must hold one global index per image")
        mask = feature_mask(features)
        ticket = C.c_int64(0)
        self._call("llfe_submit_images", descs.ctypes.data, n, mask, int(n_colors), C.c_uint64(seed & (2**64 - 1)),
                   idx.ctypes.data, self._stream(first), C.byref(ticket))
        self._inflight[ticket.value] = (n, hh, ww, mask, keep, idx, descs)
        return ticket.value

    def collect(self, ticket: int) -> list:
        n, h, w, mask, keep, nkeep, b = self._inflight[ticket]
        results, shapes, fonts = self._with_shapes(n, mask, ticket, lambda res, sh, cap, need: (
            self._lib.llfe_collect_batch(self.ctx, C.c_int64(ticket), res, sh, cap, need)))
        del self._inflight[ticket]
        return self._convert(results, shapes, n, mask, w, h, fonts)

    # ------------------------------------------------------------------ stages (device tensors)
    def _dev_batch(self, images):
        torch = _torch()
        if not _is_torch(images):
            images = torch.from_numpy(np.ascontiguousarray(images, np.uint8))
        if images.dim() == 3:
            images = images[None]
        return images.to(f"cuda:{self.device}").contiguous()

    def _dev_image(self, x, axis: int = 2):
        """One image (or mask batch) as a contiguous tensor on this device, a 2-d one made 3-d
        by a new axis ``axis`` -> (tensor, whether it was 2-d)."""
        if not _is_torch(x):
            x = _torch().from_numpy(np.ascontiguousarray(x, np.uint8))
        x = x.to(f"cuda:{self.device}").contiguous()
        squeeze = x.dim() == 2
        return (x.unsqueeze(axis) if squeeze else x), squeeze

    def _u8_map(self, fn: str, images):
        """The stage function ``fn`` (in, out, n, h, w, stream) over a batch: n x h x w u8 device
        tensor."""
        torch = _torch()
        x = self._dev_batch(images)
        n, h, w, _ = x.shape
        out = torch.empty((n, h, w), dtype=torch.uint8, device=x.device)
        self._call(fn, x.data_ptr(), out.data_ptr(), n, h, w, self._stream(x))
        return out

    def gray_blur5(self, images):
        return self._u8_map("llfe_gray_blur5", images)

    def edge_classes(self, images):
        return self._u8_map("llfe_edge_classes", images)

    def font_binary(self, images):
        """FontDetector.preprocess_image on the GPU: n x h x w u8 0/255 device tensor."""
        return self._u8_map("llfe_font_binary", images)

    def font_bits(self, images):
        """The font binary as bit rows in one kernel (llfe_font_bits): n x h x ceil(w / 64)
        int64 device tensor (the u64 words; bit x & 63 of word x >> 6 is pixel x).  ``images``:
        an N x H x W x 3 batch, or a list of separately allocated H x W x 3 device tensors of
        one size, read in place through an address table (llfe_font_bits_images)."""
        torch = _torch()
        if isinstance(images, (list, tuple)):
            ts = [t.to(f"cuda:{self.device}").contiguous() for t in images]
            n, (h, w, _) = len(ts), ts[0].shape
            if any(tuple(t.shape) != (h, w, 3) or t.dtype != torch.uint8 for t in ts):
                raise ValueError("font_bits: a list must hold H x W x 3 uint8 tensors of one size")
            out = torch.empty((n, h, (w + 63) // 64), dtype=torch.int64, device=ts[0].device)
            tab = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
            self._call("llfe_font_bits_images", tab, out.data_ptr(), n, h, w, self._stream(ts[0]))
            return out
        x = self._dev_batch(images)
        n, h, w, _ = x.shape
        out = torch.empty((n, h, (w + 63) // 64), dtype=torch.int64, device=x.device)
        self._call("llfe_font_bits", x.data_ptr(), out.data_ptr(), n, h, w, self._stream(x))
        return out

    def jpeg_reconstruct(self, coefs, descs, h: int, w: int, out=None):
        """The device half of a JPEG decode (llfe_jpeg_reconstruct): ``coefs`` an n x slot_stride
        uint8 device tensor of staged coefficients, ``descs`` the n llfe_jpeg_desc records
        (decode.stage_coefs) -> n x h x w x 3 BGR uint8 on the device, on the current stream.
        Images whose descriptor has n_comp == 0 are left untouched in ``out``.  A descriptor
        that points outside its slot raises LlfeError (LLFE_ERR_INVALID) before any launch."""
        torch = _torch()
        _dev_u8_2d("jpeg_reconstruct: coefs", coefs, "n x slot_stride")
        n, stride = coefs.shape
        if len(descs) != n:
            raise ValueError(f"jpeg_reconstruct: {len(descs)} descriptors for {n} slots")
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=coefs.device)
        if tuple(out.shape) != (n, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or \
                out.device != coefs.device:
            raise ValueError(f"jpeg_reconstruct: out must be a contiguous {(n, h, w, 3)} uint8 tensor on {coefs.device}")
        self._call("llfe_jpeg_reconstruct", coefs.data_ptr(), stride, descs, n, int(h), int(w), out.data_ptr(),
                   self._stream(coefs))
        return out

    def jpeg_reconstruct_images(self, coefs, images, descs, out, orientation=None):
        """The device half of a JPEG decode of images of any sizes (llfe_jpeg_reconstruct_images):
        ``coefs`` a 1-d uint8 device tensor of staged coefficient slots, ``images`` / ``descs`` the n
        llfe_jpeg_image / llfe_jpeg_desc records (decode.stage_coefs_images, with every
        out_offset set), ``out`` a 1-d uint8 device tensor that receives image i packed
        height x width x 3 BGR at its out_offset, on the current stream.  Images whose descriptor
        has n_comp == 0 are left untouched in ``out``.  A record that points outside its slot,
        ``coefs`` or ``out``, or into another image's result, raises LlfeError (LLFE_ERR_INVALID,
        or LLFE_ERR_CAPACITY when only ``out`` is short) before any launch.  ``orientation``: the
        EXIF orientation 1 .. 8 of every image (llfe_jpeg_reconstruct_images_oriented): image i is
        written as decode_bgr returns it, width x height x 3 for 5 .. 8; a value outside 1 .. 8 is
        refused the same way.  -> ``out``."""
        torch = _torch()
        for name, t in (("coefs", coefs), ("out", out)):
            if not (_is_torch(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1 and t.is_contiguous()):
                raise ValueError(f"jpeg_reconstruct_images: {name} must be a contiguous 1-d uint8 device tensor")
        if coefs.device.index != self.device or out.device != coefs.device:
            raise ValueError(f"jpeg_reconstruct_images: coefs on {coefs.device}, out on {out.device}, context on "
                             f"cuda:{self.device}")
        n = len(images)
        if len(descs) != n:
            raise ValueError(f"jpeg_reconstruct_images: {len(descs)} descriptors for {n} image records")
        if orientation is None:
            self._call("llfe_jpeg_reconstruct_images", coefs.data_ptr(), coefs.numel(), images, descs, n, out.data_ptr(),
                       out.numel(), self._stream(coefs))
            return out
        if len(orientation) != n:
            raise ValueError(f"jpeg_reconstruct_images: {len(orientation)} orientations for {n} image records")
        if any(not 0 <= int(o) <= 255 for o in orientation):
            raise ValueError("jpeg_reconstruct_images: an orientation is one byte")
        orient = (C.c_uint8 * n)(*[int(o) for o in orientation])
        self._call("llfe_jpeg_reconstruct_images_oriented", coefs.data_ptr(), coefs.numel(), images, descs, orient, n,
                   out.data_ptr(), out.numel(), self._stream(coefs))
        return out

    def jpeg_entropy_decode(self, records, scans, descs, h: int, w: int, slots) -> list:
        """The entropy half of a JPEG decode on the device (llfe_jpeg_entropy_decode): ``records``
        an n x record_stride uint8 device tensor of staged records, ``scans`` / ``descs`` the n
        llfe_jpeg_scan / llfe_jpeg_desc records (decode.stage_bytes), ``slots`` an
        n x slot_stride uint8 device tensor that receives quantisation tables and coefficients
        as decode.stage_coefs lays them out, on the current stream.  -> the per-image status
        list: 0 for a slot that is ready for jpeg_reconstruct, LLFE_ERR_UNSUPPORTED for an image
        that was not staged or whose scan showed an anomaly (decode it another way).  A record
        or descriptor that points outside its buffer raises LlfeError (LLFE_ERR_INVALID) before
        any launch."""
        _dev_u8_2d("jpeg_entropy_decode: records", records)
        _dev_u8_2d("jpeg_entropy_decode: slots", slots)
        n, stride = slots.shape
        if records.shape[0] != n or len(scans) != n or len(descs) != n or records.device != slots.device:
            raise ValueError(f"jpeg_entropy_decode: records, scans and descriptors for {n} slots on one device")
        status = (C.c_int32 * n)()
        self._call("llfe_jpeg_entropy_decode", records.data_ptr(), records.numel(), scans, descs, n, int(h), int(w),
                   slots.data_ptr(), stride, status, self._stream(slots))
        return list(status)

    def jpeg_entropy_decode_images(self, records, scans, descs, images, slots) -> list:
        """The entropy half of a JPEG decode of images of any sizes on the device
        (llfe_jpeg_entropy_decode_images): ``records`` a 1-d uint8 device tensor of staged records,
        ``scans`` / ``descs`` / ``images`` the n llfe_jpeg_scan / llfe_jpeg_desc / llfe_jpeg_image
        records (decode.stage_bytes_images), ``slots`` a 1-d uint8 device tensor that receives
        every image's quantisation tables and coefficients in its tight slot, as
        decode.stage_coefs_images lays them out, on the current stream.  -> the per-image status
        list: 0 for a slot that is ready for jpeg_reconstruct_images, LLFE_ERR_UNSUPPORTED for an
        image that was not staged or whose scan showed an anomaly (decode it another way).  A
        record or descriptor that points outside its buffer, or a slot that lies outside ``slots``
        or in another image's, raises LlfeError (LLFE_ERR_INVALID) before any launch."""
        torch = _torch()
        for name, t in (("records", records), ("slots", slots)):
            if not (_is_torch(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1 and t.is_contiguous()):
                raise ValueError(f"jpeg_entropy_decode_images: {name} must be a contiguous 1-d uint8 device tensor")
        if slots.device.index != self.device or records.device != slots.device:
            raise ValueError(f"jpeg_entropy_decode_images: records on {records.device}, slots on {slots.device}, "
                             f"context on cuda:{self.device}")
        n = len(images)
        if len(scans) != n or len(descs) != n:
            raise ValueError(f"jpeg_entropy_decode_images: {len(scans)} scan records and {len(descs)} descriptors for "
                             f"{n} image records")
        status = (C.c_int32 * n)()
        self._call("llfe_jpeg_entropy_decode_images", records.data_ptr(), records.numel(), scans, descs, images, n,
                   slots.data_ptr(), slots.numel(), status, self._stream(slots))
        return list(status)

    def png_decode(self, records, descs, h: int, w: int, out, raw=None) -> list:
        """PNG decode on the device (llfe_png_decode_device): ``records`` an n x record_stride
        uint8 device tensor of staged deflate streams, ``descs`` the n llfe_png_desc records
        (decode.stage_png), ``out`` the n x h x w x 3 BGR uint8 device tensor, on the current
        stream.  ``raw`` (n x raw_stride uint8 on the device, raw_stride a multiple of 16 that
        holds h * (w * 4 + 1) bytes; allocated here when None) receives the inflated filtered
        rows.  -> the per-image status list: 0 for an image whose pixels are in ``out``,
        LLFE_ERR_UNSUPPORTED for one that was not staged or whose stream showed an anomaly (its
        place in ``out`` is undefined: decode it another way).  A descriptor that points outside
        its record raises LlfeError (LLFE_ERR_INVALID) before any launch."""
        torch = _torch()
        _dev_u8_2d("png_decode: records", records, "n x record_stride")
        n = records.shape[0]
        if len(descs) != n:
            raise ValueError(f"png_decode: {len(descs)} descriptors for {n} records")
        if not (_is_torch(out) and tuple(out.shape) == (n, h, w, 3) and out.dtype == torch.uint8 and out.is_contiguous()
                and out.device == records.device):
            raise ValueError(f"png_decode: out must be a contiguous {(n, h, w, 3)} uint8 tensor on {records.device}")
        if raw is None:
            need = max([d.raw_bytes for d in descs], default=0)
            raw = torch.empty((n, max(16, (need + 15) & ~15)), dtype=torch.uint8, device=records.device)
        if not (_is_torch(raw) and raw.dim() == 2 and raw.shape[0] == n and raw.dtype == torch.uint8 and
                raw.is_contiguous() and raw.device == records.device):
            raise ValueError(f"png_decode: raw must be a contiguous {n} x raw_stride uint8 tensor on {records.device}")
        status = (C.c_int32 * n)()
        self._call("llfe_png_decode_device", records.data_ptr(), records.numel(), descs, n, int(h), int(w),
                   raw.data_ptr(), raw.shape[1], out.data_ptr(), status, self._stream(records))
        return list(status)

    def font_detect(self, images, binary=None, regions=False) -> list:
        """FontDetector.detect_font's pixel work on the GPU (llfe_font_detect): per image
        the external contours of the font binary (or of ``binary``, n x h x w, nonzero =
        foreground), the text regions among their bounding boxes, the largest one and the
        exact gray sum over it.  ``images``: N x H x W x 3 BGR, numpy or device tensor (None
        with a ``binary``: no gray sums).  -> list of dicts n_contours, n_regions, x, y,
        width, height, gray_sum and, with ``regions=True``, regions: [(x, y, w, h)] in
        findContours order.  No mask or image comes back to the host."""
        torch = _torch()
        if images is None and binary is None:
            raise ValueError("font_detect needs images or a binary")
        x = self._dev_batch(images) if images is not None else None
        b = None
        if binary is not None:
            if _is_torch(binary) and binary.dtype != torch.uint8:
                raise ValueError(f"expected a uint8 binary, got {binary.dtype}")
            b, _ = self._dev_image(binary, axis=0)
            if b.dim() != 3 or (x is not None and tuple(b.shape) != tuple(x.shape[:3])):
                raise ValueError(f"binary {tuple(b.shape)} does not match the images")
        n, h, w = (x if x is not None else b).shape[:3]
        res = (L.LlfeFontResult * max(n, 1))()
        need = C.c_int64(0)
        cap = max(4096, 256 * n) if regions else 0
        while True:
            reg = np.empty((cap, 4), np.int32) if regions else None
            with self._lock:
                rc = self._lib.llfe_font_detect(self.ctx, x.data_ptr() if x is not None else None,
                                                b.data_ptr() if b is not None else None, n, h, w, res,
                                                reg.ctypes.data if regions else None, cap, C.byref(need),
                                                self._stream(x if x is not None else b))
            if rc == L.LLFE_ERR_CAPACITY and regions and need.value > cap:  # grown once: need is exact
                cap = int(need.value)
                continue
            self._chk(rc)
            break
        out = []
        for i in range(n):
            d = _font_dict(res[i])
            if regions:
                o = int(res[i].region_offset)
                d["regions"] = [tuple(v) for v in reg[o:o + d["n_regions"]].tolist()]
            out.append(d)
        return out

    def text_binary(self, image):
        """TextExtractor.preprocess_image on the GPU (text_extractor.py:15-46): one
        H x W [x C] uint8 image (C = 1, 3 BGR or 4 BGRA) -> (out_h x out_w 0/255 device
        tensor, Otsu threshold)."""
        torch = _torch()
        x, _ = self._dev_image(image)
        h, w, ch = x.shape
        oh, ow = text_size(h, w)
        out = torch.empty((oh, ow), dtype=torch.uint8, device=x.device)
        t = C.c_int32(0)
        self._call("llfe_text_binary", x.data_ptr(), h, w, ch, out.data_ptr(), C.byref(t),
                                             self._stream(x))
        return out, int(t.value)

    def shape_mask(self, images):
        return self._u8_map("llfe_shape_mask", images)

    def canny(self, images):
        """Canny(blur5(gray), 50, 150) of the shapes path, before its dilation: n x h x w
        u8 0/255 device tensor."""
        return self._u8_map("llfe_canny", images)

    def hysteresis(self, classes, tile_flags=True):
        """The hysteresis of canny / shape_mask on caller class maps: an n x h x w (or
        h x w) host u8 array of 0 (weak) / 1 (none) / 2 (strong) -> (edges, mask) as
        n x h x w 0/255 numpy arrays, mask = edges dilated 3 x 3.  ``tile_flags``: list
        only the 64 x 64 tiles with a candidate (as after the stencil) or every tile."""
        c = np.ascontiguousarray(classes, np.uint8)
        if c.ndim == 2:
            c = c[None]
        n, h, w = c.shape
        edges, mask = np.empty_like(c), np.empty_like(c)
        self._call("llfe_hysteresis", c.ctypes.data, n, h, w, 1 if tile_flags else 0, edges.ctypes.data,
                   mask.ctypes.data)
        return edges, mask

    @staticmethod
    def _unpack_words(words, layout):
        """Packed mask words at a shapes layout's offsets -> list of h x w u8 0 / 255 arrays."""
        recs, _, passes = layout
        out = []
        for r in recs:
            h, w = r["height"], r["width"]
            wpr = (w + 63) // 64
            first = passes[r["pass"]]["first_word"] + r["word_offset"]
            rows = words[first:first + h * wpr].reshape(h, wpr)
            bits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :w]
            out.append(bits * np.uint8(255))
        return out

    def shape_masks_images(self, images) -> list:
        """shape_mask for a list of images of any sizes (as process_images takes them, no
        preprocessing) through the one-pass shapes route (llfe_shape_bits_images): -> list of
        h x w u8 0 / 255 numpy arrays in input order."""
        n = len(images)
        if n == 0:
            return []
        descs, keep, _, _, first = _image_descs(images, self.device)
        layout = shapes_images_layout(keep, device=self.device)
        total = layout[2][-1]["first_word"] + layout[2][-1]["words"]
        words = np.zeros(total, np.uint64)
        self._call("llfe_shape_bits_images", descs.ctypes.data, n, words.ctypes.data, total, self._stream(first))
        del keep
        return self._unpack_words(words, layout)

    def shadow_stats_images(self, images):
        """shadow_stats for a list of images of any sizes through the one-pass route
        (llfe_shadow_stats_images): -> (sums, counts) np.uint64[n]."""
        n = len(images)
        sums, cnts = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        if n:
            descs, keep, _, _, first = _image_descs(images, self.device)
            self._call("llfe_shadow_stats_images", descs.ctypes.data, n, sums.ctypes.data, cnts.ctypes.data,
                       self._stream(first))
            del keep
        return sums, cnts

    def hysteresis_images(self, class_maps, tile_flags=True) -> list:
        """hysteresis for a list of h x w host class maps of any sizes in one ragged pass
        (llfe_hysteresis_images): -> list of (edges, mask) h x w 0 / 255 numpy arrays."""
        maps = [np.ascontiguousarray(c, np.uint8) for c in class_maps]
        n = len(maps)
        if n == 0:
            return []
        if any(c.ndim != 2 for c in maps):
            raise ValueError("class maps must be h x w")
        layout = shapes_images_layout([np.zeros(c.shape + (3,), np.uint8) for c in maps], device=self.device)
        total = layout[2][-1]["first_word"] + layout[2][-1]["words"]
        ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in maps])
        hs = np.array([c.shape[0] for c in maps], np.int32)
        ws = np.array([c.shape[1] for c in maps], np.int32)
        edges, mask = np.zeros(total, np.uint64), np.zeros(total, np.uint64)
        self._call("llfe_hysteresis_images", ptrs, hs.ctypes.data, ws.ctypes.data, n, 1 if tile_flags else 0,
                   edges.ctypes.data, mask.ctypes.data, total)
        return list(zip(self._unpack_words(edges, layout), self._unpack_words(mask, layout)))

    def dilate3(self, masks):
        """dilate(masks, ones(3, 3)) of an n x h x w (or h x w) u8 batch on the GPU."""
        torch = _torch()
        x, _ = self._dev_image(masks, axis=0)
        n, h, w = x.shape
        out = torch.empty_like(x)
        self._call("llfe_dilate3", x.data_ptr(), out.data_ptr(), n, h, w, self._stream(x))
        return out

    def find_contours_gpu(self, mask: np.ndarray) -> list:
        """findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) of one host u8 mask on the GPU
        contour path (the one llfe_process_batch uses) -> list of (n,2) int32, cv2 order."""
        m = np.ascontiguousarray(mask, np.uint8)
        h, w = m.shape
        cap = 1 << 16
        while True:
            pts = np.empty((cap, 2), np.int32)
            offs = np.empty(cap + 1, np.int32)
            need = C.c_int64(0)
            with self._lock:
                nc = self._lib.llfe_find_contours_gpu(self.ctx, m.ctypes.data, h, w, pts.ctypes.data, cap,
                                                      offs.ctypes.data, cap + 1, C.byref(need))
            if nc == L.LLFE_ERR_CAPACITY:
                cap = max(int(need.value), cap * 2)
                continue
            self._chk(min(nc, 0))
            return [pts[offs[i]:offs[i + 1]].copy() for i in range(nc)]

    def shapes_from_masks_gpu(self, masks: np.ndarray):
        """analyze_shapes' records for n host u8 masks (n x h x w) on the GPU contour path
        -> (list of per-image shape dict lists, n_contours np.int32[n])."""
        m = np.ascontiguousarray(masks, np.uint8)
        n, h, w = m.shape
        cap = max(64, 16 * n)
        while True:
            arr = (L.LlfeShape * cap)()
            ns = np.zeros(n, np.int32)
            nc = np.zeros(n, np.int32)
            need = C.c_int64(0)
            with self._lock:
                rc = self._lib.llfe_shapes_from_masks_gpu(self.ctx, m.ctypes.data, n, h, w, arr, cap, ns.ctypes.data,
                                                          nc.ctypes.data, C.byref(need))
            if rc == L.LLFE_ERR_CAPACITY:
                cap = int(need.value)
                continue
            self._chk(rc)
            out, k = [], 0
            for i in range(n):
                out.append([_shape_dict(s) for s in arr[k:k + ns[i]]])
                k += int(ns[i])
            return out, nc

    def shadow_stats(self, images):
        x = self._dev_batch(images)
        n, h, w, _ = x.shape
        sums = np.zeros(n, np.uint64)
        cnts = np.zeros(n, np.uint64)
        self._call("llfe_shadow_stats", x.data_ptr(), sums.ctypes.data, cnts.ctypes.data, n, h, w,
                                              self._stream(x))
        return sums, cnts

    def color_unique(self, images, seed=0, noise=None, index_base=0):
        """-> (keys device tensor n x h*w int32 view of u32, n_unique np.int64[n])"""
        torch = _torch()
        x = self._dev_batch(images)
        n, h, w, _ = x.shape
        nz = None
        if noise is not None:
            nz = torch.as_tensor(np.ascontiguousarray(noise, np.int8)).to(x.device).contiguous()
        keys = torch.empty((n, h * w), dtype=torch.int32, device=x.device)
        nu = np.zeros(n, np.int64)
        b = L.LlfeBatch(C.c_void_p(x.data_ptr()), n, h, w, 1, C.c_void_p(nz.data_ptr()) if nz is not None else None,
                        1, 0, index_base)
        self._call("llfe_color_unique", C.byref(b), C.c_uint64(seed), keys.data_ptr(),
                                              nu.ctypes.data, self._stream(x))
        return keys, nu

    def color_unique_images(self, images, seed=0, noise=None, index_base=0) -> list:
        """llfe_color_unique for a list of images of any sizes (as process_images takes them,
        no preprocessing) in one colour pass: -> [(sorted unique keys np.uint32[n_unique],
        n_unique)] in input order.  ``noise``: one parity-noise array per image, or None."""
        torch = _torch()
        n = len(images)
        if n == 0:
            return []
        descs, keep, hs, ws, first = _image_descs(images, self.device)
        if noise is not None:
            nz = [self._noise_view(noise[i], 1, hs[i], ws[i]) for i in range(n)]
            descs["noise"], descs["noise_on_device"] = [v[0] or 0 for v in nz], [v[1] for v in nz]
            keep.append(nz)
        stride = (max(h * w for h, w in zip(hs, ws)) + 3) & ~3
        keys = torch.empty((n, stride), dtype=torch.int32, device=f"cuda:{self.device}")
        nu = np.zeros(n, np.int64)
        self._call("llfe_color_unique_images", descs.ctypes.data, n, C.c_uint64(seed & (2**64 - 1)), index_base,
                   keys.data_ptr(), stride, nu.ctypes.data, self._stream(first))
        host = keys.cpu().numpy().view(np.uint32)
        del keep
        return [(host[i, :nu[i]].copy(), int(nu[i])) for i in range(n)]

    def kmeans(self, keys, n_points, n_colors=5, seed=0, index_base=0):
        """keys: device int32 tensor (n, stride) of packed RGB keys; n_points np.int64[n]."""
        n = keys.shape[0]
        n_points = np.ascontiguousarray(n_points, np.int64)
        res = (L.LlfeImageResult * max(n, 1))()
        self._call("llfe_kmeans", keys.data_ptr(), keys.shape[1], n_points.ctypes.data, n, n_colors,
                                        C.c_uint64(seed), index_base, res, self._stream(keys))
        out = []
        for i in range(n):
            r = res[i]
            k = r.n_colors
            centers = np.array([[r.centers_rgb[j][c] for c in range(3)] for j in range(k)], np.uint8).reshape(-1, 3)
            out.append((centers, np.array([r.counts[j] for j in range(k)], np.int64), float(r.compactness)))
        return out

    def kmeans_attempts(self, n, k=5):
        """Diagnostics (llfe_kmeans_attempts): the 10 k-means attempts of each of the first n
        images of the last k-means launch on this context -- the last chunk of process() /
        process_images(), a kmeans() call on caller keys, or the ticket submit() / submit_images()
        issued last (refused until every ticket is collected) -- for n_colors <= 5
        -> list of n lists of dicts (pp_centers, centers float32 5 x 3 before the uint8
        truncation, counts, iters, compactness; rows past K unused).
        k > 5 (llfe_kmeans_attempts_k): the same for a launch with n_colors <= k, k rows each
        (rows past an image's K zero)."""
        if k > 5:
            pp = np.zeros((n, 10, k, 3), np.float32)
            cen = np.zeros((n, 10, k, 3), np.float32)
            cnt = np.zeros((n, 10, k), np.int32)
            it = np.zeros((n, 10), np.int32)
            comp = np.zeros((n, 10), np.float64)
            self._call("llfe_kmeans_attempts_k", n, k, pp.ctypes.data, cen.ctypes.data, cnt.ctypes.data,
                       it.ctypes.data, comp.ctypes.data)
            return [[{"pp_centers": pp[i, a], "centers": cen[i, a], "counts": cnt[i, a].astype(np.int64),
                      "iters": int(it[i, a]), "compactness": float(comp[i, a])} for a in range(10)]
                    for i in range(n)]
        out = (L.LlfeKmeansAttempt * max(n * 10, 1))()
        self._call("llfe_kmeans_attempts", n, out)
        recs = []
        for i in range(n):
            row = []
            for a in range(10):
                r = out[i * 10 + a]
                row.append({"pp_centers": np.array([[r.pp_centers[k][j] for j in range(3)] for k in range(5)], np.float32),
                            "centers": np.array([[r.centers[k][j] for j in range(3)] for k in range(5)], np.float32),
                            "counts": np.array(list(r.counts), np.int64), "iters": int(r.iters),
                            "compactness": float(r.compactness)})
            recs.append(row)
        return recs

    def resize_lanczos_pil(self, image, out_w, out_h, box=None):
        """Pillow LANCZOS resize of one H x W x C uint8 image (torch GPU tensor or numpy)."""
        torch = _torch()
        x, _ = self._dev_image(image)
        h, w, ch = x.shape
        out = torch.empty((out_h, out_w, ch), dtype=torch.uint8, device=x.device)
        bx = None
        if box is not None:
            bx = (C.c_double * 4)(*[float(v) for v in box])
        self._call("llfe_resize_lanczos_pil", x.data_ptr(), h, w, ch, out.data_ptr(), out_h, out_w,
                                                    bx, self._stream(x))
        return out


    def reduce_pil(self, image, fx, fy):
        torch = _torch()
        x, _ = self._dev_image(image)
        h, w, ch = x.shape
        out = torch.empty(((h + fy - 1) // fy, (w + fx - 1) // fx, ch), dtype=torch.uint8, device=x.device)
        self._call("llfe_reduce_pil", x.data_ptr(), h, w, ch, fx, fy, out.data_ptr(),
                                            self._stream(x))
        return out

    def resize_cv(self, image, out_w, out_h, interpolation):
        """cv2.resize(image, (out_w, out_h), interpolation) of one H x W [x C] uint8 image
        (validate_and_preprocess_image, utils.py:118-143); interpolation is an OpenCV
        code or one of "linear" / "area" / "lanczos4"."""
        torch = _torch()
        code = CV_INTER[interpolation] if isinstance(interpolation, str) else int(interpolation)
        x, squeeze = self._dev_image(image)
        h, w, ch = x.shape
        out = torch.empty((out_h, out_w, ch), dtype=torch.uint8, device=x.device)
        self._call("llfe_resize_cv", x.data_ptr(), h, w, ch, out.data_ptr(), out_h, out_w, code,
                                           self._stream(x))
        return out[:, :, 0] if squeeze else out

    def thumbnail_pil(self, image, max_w=1920, max_h=1080):
        """PIL thumbnail((max_w, max_h), LANCZOS) of one H x W x C uint8 image."""
        torch = _torch()
        x, squeeze = self._dev_image(image)
        h, w, ch = x.shape
        out = torch.empty(h * w * ch, dtype=torch.uint8, device=x.device)
        oh, ow = C.c_int32(0), C.c_int32(0)
        self._call("llfe_thumbnail_pil", x.data_ptr(), h, w, ch, max_w, max_h, out.data_ptr(),
                                               out.numel(), C.byref(oh), C.byref(ow), self._stream(x))
        out = out[: oh.value * ow.value * ch].view(oh.value, ow.value, ch)
        return out[:, :, 0] if squeeze else out

    def thumbnail_pil_batch(self, images, max_w=1920, max_h=1080):
        """PIL thumbnail((max_w, max_h), LANCZOS) of N same-size H x W x 3 uint8 images
        (N x H x W x 3 array / tensor) in one llfe_thumbnail_pil_batch call."""
        torch = _torch()
        x, _ = self._dev_image(images)
        n, h, w, ch = x.shape
        plan = thumbnail_size(w, h, max_w, max_h)
        ow, oh = plan if plan else (w, h)
        out = torch.empty((n, oh, ow, ch), dtype=torch.uint8, device=x.device)
        ro, co = C.c_int32(0), C.c_int32(0)
        self._call("llfe_thumbnail_pil_batch", x.data_ptr(), n, h, w, ch, max_w, max_h, out.data_ptr(),
                                                     out.numel(), C.byref(ro), C.byref(co), self._stream(x))
        assert (ro.value, co.value) == (oh, ow)
        return out

    def thumbnail_pil_images(self, images, max_w=1920, max_h=1080) -> list:
        """PIL thumbnail((max_w, max_h), LANCZOS) of a list of H x W x 3 uint8 images of any
        sizes -- numpy arrays and / or torch tensors, host or GPU, rows may be strided -- in one
        llfe_thumbnail_pil_images call.  -> one device tensor H' x W' x 3 per image, in input
        order, each a view into one packed uint8 tensor."""
        torch = _torch()
        n = len(images)
        if n == 0:
            return []
        descs, keep, _, _, first = _image_descs(images, self.device)
        outs = (L.LlfeThumbOut * n)()
        total = C.c_int64(0)
        rc = self._lib.llfe_thumbnail_images_layout(descs.ctypes.data, n, int(max_w), int(max_h), outs, C.byref(total))
        if rc < 0:
            raise L.LlfeError(rc, "invalid thumbnail batch")
        packed = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        self._call("llfe_thumbnail_pil_images", descs.ctypes.data, n, int(max_w), int(max_h), packed.data_ptr(),
                   packed.numel(), outs, self._stream(first))
        del keep
        return [packed[o.offset: o.offset + o.height * o.width * 3].view(o.height, o.width, 3) for o in outs]

    def _resize_images(self, fn: str, descs, first, arg, out_sizes, host: bool = False):
        """llfe_preprocess_images / llfe_resize_cv_images over the records ``descs`` (``arg``: the
        mode / the address of the size triples; the caller keeps the images alive) -> (views into
        one packed device tensor, the call's llfe_resize_out records)."""
        torch = _torch()
        n = len(descs)
        outs = (L.LlfeResizeOut * max(n, 1))()
        # the packed size: every result at a multiple of 16 (a bad size is the call's to refuse)
        cap = sum(16 + 3 * oh * ow for oh, ow in out_sizes) if n else 0
        packed = torch.empty(max(cap, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        self._call(fn, descs.ctypes.data, n, arg, packed.data_ptr(), packed.numel(), outs, self._stream(first))
        if host:  # one D2H of the packed results
            packed = packed.cpu().numpy()
            return [packed[o.offset: o.offset + o.height * o.width * 3].reshape(o.height, o.width, 3)
                    for o in outs[:n]], outs
        return [packed[o.offset: o.offset + o.height * o.width * 3].view(o.height, o.width, 3) for o in outs[:n]], outs

    def preprocess_images(self, images, preprocessing: str = "auto", host: bool = False) -> list:
        """validate_and_preprocess_image's resize (``preprocessing``: none / auto / high_quality /
        performance) of a list of H x W x 3 BGR uint8 images of any sizes -- numpy arrays and / or
        torch tensors, host or GPU, rows may be strided -- in one llfe_preprocess_images call.
        -> one device tensor H' x W' x 3 per image, in input order, each a view into one packed
        uint8 tensor at a multiple of 16 bytes; an image the rule leaves is copied.  The bytes are
        those of ``resize_cv`` of each image.  ``host=True``: numpy arrays instead, from one
        device-to-host copy of the packed tensor."""
        mode = _pre_mode(preprocessing)
        if len(images) == 0:
            return []
        descs, keep, _, _, first = _image_descs(images, self.device)
        res = self._preprocess_descs(descs, first, mode, host)
        del keep
        return res

    def _preprocess_descs(self, descs, first, mode: int, host: bool = False) -> list:
        """preprocess_images over prepared records: the layout (host only), then the call."""
        n = len(descs)
        lay = (L.LlfeResizeOut * n)()
        total = C.c_int64(0)
        rc = self._lib.llfe_preprocess_images_layout(descs.ctypes.data, n, mode, lay, C.byref(total))
        if rc < 0:  # (the call itself names the image)
            self._call("llfe_preprocess_images", descs.ctypes.data, n, mode, None, 0, lay, None)
            raise L.LlfeError(rc, "invalid preprocessing batch")  # pragma: no cover
        return self._resize_images("llfe_preprocess_images", descs, first, mode, [(o.height, o.width) for o in lay],
                                   host)[0]

    def resize_cv_images(self, images, sizes) -> list:
        """cv2.resize of a list of H x W x 3 uint8 images of any sizes in one llfe_resize_cv_images
        call; ``sizes``: one (out_w, out_h, interpolation) per image, as ``resize_cv`` takes them
        ("linear" / "area" / "lanczos4" or the OpenCV code).  -> device tensors as
        ``preprocess_images`` returns them."""
        if len(sizes) != len(images):
            raise ValueError("sizes must hold one (out_w, out_h, interpolation) per image")
        if len(images) == 0:
            return []
        s3 = np.ascontiguousarray([(int(oh), int(ow), CV_INTER[it] if isinstance(it, str) else int(it))
                                   for ow, oh, it in sizes], dtype=np.int32)
        out_sizes = [(max(int(oh), 0), max(int(ow), 0)) for ow, oh, _ in sizes]
        descs, keep, _, _, first = _image_descs(images, self.device)
        res = self._resize_images("llfe_resize_cv_images", descs, first, s3.ctypes.data, out_sizes)[0]
        del keep
        return res


_FONT_FIELDS = ("n_contours", "n_regions", "x", "y", "width", "height", "gray_sum")
# "gpu_force_fallback": diagnostic GPU mode whose chunks all take the host fallback
CONTOUR_MODES = {"host": 0, "gpu": 1, "gpu_force_fallback": 2}
CV_INTER = {"linear": 1, "cubic": 2, "area": 3, "lanczos4": 4}
PRE_MODES = {"none": 0, "auto": 1, "high_quality": 2, "performance": 3}
_INTER_NAME = {1: "INTER_LINEAR", 3: "INTER_AREA", 4: "INTER_LANCZOS4"}


def preprocess_size(w, h, mode):
    """validate_and_preprocess_image's size rule (utils.py:118-143) through the ABI:
    -> (new_w, new_h, interpolation code) or None when the mode does not resize."""
    if mode not in PRE_MODES:
        return None
    ow, oh, it = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = L.lib().llfe_preprocess_size(w, h, PRE_MODES[mode], C.byref(ow), C.byref(oh), C.byref(it))
    if rc < 0:
        raise L.LlfeError(rc, "invalid preprocessing geometry")
    return (ow.value, oh.value, it.value) if rc == 1 else None


def thumbnail_size(w, h, max_w=1920, max_h=1080):
    """-> (new_w, new_h) or None when PIL's thumbnail would not resize."""
    ow, oh = C.c_int32(0), C.c_int32(0)
    rc = L.lib().llfe_thumbnail_size(w, h, max_w, max_h, C.byref(ow), C.byref(oh))
    if rc < 0:
        raise L.LlfeError(rc, "invalid thumbnail geometry")
    return (ow.value, oh.value) if rc == 1 else None


# ---------------------------------------------------------------------- host-only geometry
def find_contours(mask: np.ndarray) -> list:
    """findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) -> list of (n,2) int32."""
    lib = L.lib()
    m = np.ascontiguousarray(mask, np.uint8)
    h, w = m.shape
    cap = 1 << 16
    while True:
        pts = np.empty((cap, 2), np.int32)
        offs = np.empty(cap + 1, np.int32)
        need = C.c_int64(0)
        nc = lib.llfe_find_contours(m.ctypes.data, h, w, pts.ctypes.data, cap, offs.ctypes.data, cap + 1,
                                    C.byref(need))
        if nc == L.LLFE_ERR_CAPACITY:
            cap = max(int(need.value), cap * 2)
            continue
        if nc < 0:
            raise L.LlfeError(nc, "llfe_find_contours failed")
        return [pts[offs[i]:offs[i + 1]].copy() for i in range(nc)]


def _contour_xy(contour) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(contour).reshape(-1, 2), np.int32)


def border_radius(contour, epsilon_factor=0.02) -> float:
    p = _contour_xy(contour)
    return float(L.lib().llfe_border_radius(p.ctypes.data, len(p), epsilon_factor))


def classify_contour(contour):
    p = _contour_xy(contour)
    s = L.LlfeShape()
    rc = L.lib().llfe_classify_contour(p.ctypes.data, len(p), C.byref(s))
    if rc < 0:
        raise L.LlfeError(rc, "llfe_classify_contour failed")
    if rc == 0:
        return None
    return _shape_dict(s)


def shapes_from_mask(mask: np.ndarray) -> list:
    lib = L.lib()
    m = np.ascontiguousarray(mask, np.uint8)
    h, w = m.shape
    cap = 1024
    while True:
        arr = (L.LlfeShape * cap)()
        nc = C.c_int32(0)
        n = lib.llfe_shapes_from_mask(m.ctypes.data, h, w, arr, cap, C.byref(nc))
        if n == L.LLFE_ERR_CAPACITY:
            cap *= 4
            continue
        if n < 0:
            raise L.LlfeError(n, "llfe_shapes_from_mask failed")
        return [_shape_dict(s) for s in arr[:n]]
