"""Host-side image decoding with cv2.imdecode(buf, IMREAD_COLOR) semantics.

Decoding stays on the host (north star); the reference decodes with OpenCV at
image_processor.py:208-211 and utils.py:108-109.  IMREAD_COLOR yields an 8-bit,
3-channel BGR array: alpha is dropped (not composited), grey and palette images are
expanded, 16-bit samples are scaled by >> 8, and JPEG EXIF orientation is applied.

PNG and JPEG go through libllfe's native host decoders (``llfe_decode_batch``:
csrc/png_decode.cpp, and csrc/jpeg_decode.cpp over the system libjpeg-turbo with
OpenCV's settings), fanned out over native threads; what they hand back (interlaced
PNG, CMYK JPEG, EXIF-rotated JPEG, other formats) is decoded with Pillow.  Images
above ``MAX_PIXELS`` (cv2's CV_IO_MAX_IMAGE_PIXELS, 2^30) fail like cv2.imdecode does.

``decode_batch_device`` (opt-in, at the end of this module) returns the same batch in device
memory: for JPEG the host stops after the entropy half and csrc/jpeg_images.hip reconstructs;
with ``entropy="device"`` baseline files are entropy-decoded on the device too (csrc/jpeg_huff.hip);
with ``png="device"`` 8-bit RGB / RGBA PNGs are inflated, unfiltered and converted there
(csrc/png_inflate.hip).  ``decode_images_device`` (opt-in too) is decode_many's device form for
images that each have their own size: the JPEG coefficient path over tight slots, one launch of
csrc/jpeg_images.hip, the results views into one packed device tensor; with ``entropy="device"``
the tight slots are filled on the device too (csrc/jpeg_huff.hip) from the files' bytes.
"""
from __future__ import annotations

import io
import threading as _threading

import numpy as np


class DecodeError(ValueError):
    pass


_PNG_SIG = b"\x89PNG\r\n\x1a\n"
MAX_PIXELS = 1 << 30  # cv2 CV_IO_MAX_IMAGE_PIXELS (libllfe: LLFE_MAX_PIXELS)
_ERR_CAPACITY = -3


def _is_native(b) -> bool:
    return b[:8] == _PNG_SIG or b[:3] == b"\xff\xd8\xff"


def _native(blobs, h, w, out, threads) -> list:
    """libllfe's host decoders (PNG / JPEG, llfe_decode_batch) over all blobs into
    out[i]; other formats get LLFE_ERR_UNSUPPORTED.  Returns the per-image status list."""
    from . import _lib

    ptrs, sizes, status, keep = _blob_table(blobs, _is_native)
    _lib.lib().llfe_decode_batch(ptrs, sizes, len(blobs), h, w, out.ctypes.data, status, int(threads))
    del keep
    return list(status)


def _blob_table(blobs, take=None):
    """The arguments every batch entry point of libllfe takes for n blobs: (pointer array, size
    array, zeroed int32 status array, keep-alive list).  A blob that ``take`` refuses gets a NULL
    pointer."""
    import ctypes as C

    n = len(blobs)
    keep = [C.c_char_p(b) if take is None or take(b) else None for b in blobs]
    ptrs = (C.c_void_p * n)(*[C.cast(k, C.c_void_p) if k is not None else None for k in keep])
    return ptrs, (C.c_uint64 * n)(*[len(b) for b in blobs]), (C.c_int32 * n)(), keep


def decoder_info() -> str:
    """Codecs the native decoders run on this host: "png=libdeflate|zlib;jpeg=..."."""
    import ctypes as C

    from . import _lib

    buf = C.create_string_buffer(128)
    _lib.lib().llfe_decoder_info(buf, 128)
    return buf.value.decode()


def _image_size(b):
    """(h, w) of a PNG / JPEG from its header, None for other formats or unreadable
    headers; DecodeError above MAX_PIXELS (cv2.imdecode returns None there)."""
    import ctypes as C

    from . import _lib

    if not _is_native(b):
        return None
    w, h = C.c_int32(), C.c_int32()
    rc = _lib.lib().llfe_image_info(b, len(b), C.byref(w), C.byref(h))
    if rc == _ERR_CAPACITY:
        raise DecodeError(f"Failed to decode image: {w.value}x{h.value} exceeds {MAX_PIXELS} pixels")
    if rc != 0:
        return None
    return h.value, w.value


# Serialises _pillow_open: warnings.catch_warnings saves / restores the process-global
# filter list and the retry below swaps Image.MAX_IMAGE_PIXELS, so two decode threads
# inside it at once could leave either changed.  Image.open only parses the header.
_PIL_OPEN_LOCK = _threading.Lock()


def _pillow_open(Image, image_bytes: bytes):
    """Image.open under cv2.imdecode's size limit (MAX_PIXELS) instead of Pillow's
    decompression-bomb guard (2 x MAX_IMAGE_PIXELS, ~179 MP by default), leaving that
    process-global guard and the warning filters as they were: the warning between the
    two Pillow limits is suppressed locally, and only an image Pillow refuses outright is
    opened again with the limit raised for that one call.  All of it under one lock, so
    concurrent decode threads neither interleave the filter save / restore nor see each
    other's raised limit."""
    import warnings

    with _PIL_OPEN_LOCK, warnings.catch_warnings():
        warnings.simplefilter("ignore", Image.DecompressionBombWarning)
        try:
            return Image.open(io.BytesIO(image_bytes))
        except Image.DecompressionBombError:
            pass
        old = Image.MAX_IMAGE_PIXELS
        Image.MAX_IMAGE_PIXELS = MAX_PIXELS  # (the MAX_PIXELS check of the caller still applies)
        try:
            return Image.open(io.BytesIO(image_bytes))
        finally:
            Image.MAX_IMAGE_PIXELS = old


def decode_bgr(image_bytes: bytes) -> np.ndarray:
    """-> H x W x 3 uint8 BGR, or raises DecodeError (cv2.imdecode returned None)."""
    from PIL import Image, ImageOps, UnidentifiedImageError

    if not image_bytes:
        raise DecodeError("Failed to decode image")
    hw = _image_size(image_bytes)
    if hw is not None:  # native PNG / JPEG path; anything it does not take goes through Pillow
        out = np.empty((1, hw[0], hw[1], 3), np.uint8)
        if _native([image_bytes], hw[0], hw[1], out, 1)[0] == 0:
            return out[0]
    # cv2.imdecode accepts up to CV_IO_MAX_IMAGE_PIXELS; Pillow's decompression-bomb
    # check would refuse images above 2 * MAX_IMAGE_PIXELS (~179 MP by default) at open
    try:
        im = _pillow_open(Image, image_bytes)
        if im.width * im.height > MAX_PIXELS:
            raise DecodeError(f"Failed to decode image: {im.width}x{im.height} exceeds {MAX_PIXELS} pixels")
        im.load()
    except (UnidentifiedImageError, OSError, ValueError, SyntaxError, Image.DecompressionBombError) as e:
        if isinstance(e, DecodeError):
            raise
        raise DecodeError("Failed to decode image") from e
    if im.format == "JPEG":
        im = ImageOps.exif_transpose(im)
    mode = im.mode
    if mode in ("I;16", "I;16B", "I;16L", "I"):
        a = np.asarray(im)
        if a.dtype != np.uint16:
            a = np.clip(a, 0, 65535).astype(np.uint16)
        g = (a >> 8).astype(np.uint8)
        rgb = np.repeat(g[:, :, None], 3, axis=2)
    elif mode == "RGB":
        rgb = np.asarray(im)
    elif mode in ("RGBA", "RGBX", "RGBa"):
        rgb = np.asarray(im)[:, :, :3]
    elif mode in ("L", "1", "P", "PA", "LA", "CMYK", "YCbCr", "HSV", "LAB", "F"):
        if mode == "LA":
            im = im.getchannel("L")
        elif mode == "PA":
            im = im.convert("RGBA")
        rgb = np.asarray(im.convert("RGB"))[:, :, :3]
    else:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


# ---------------------------------------------------------------------------- batches
# at ~10k 1080p images/s per node the host decode, not the GPU, is
# the end-to-end bound, so decoding fans out over a thread pool (Pillow's codecs release
# the GIL) and writes straight into the NHWC batch that goes to the device.
_POOL = None
_POOL_LOCK = _threading.Lock()


def usable_cores() -> int:
    """CPUs this process may run on (affinity mask, capped by a cgroup v2 cpu.max quota)."""
    import os

    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def default_decode_threads() -> int:
    """The rank's share of the host cores: the set placement.bind() pinned it to
    (LLFE_RANK_CPUS), else usable cores / LOCAL_WORLD_SIZE (one process per GPU shares the
    node's cores); LLFE_DECODE_THREADS overrides."""
    import os

    env = os.environ.get("LLFE_DECODE_THREADS")
    if env and int(env) > 0:
        return int(env)
    rank_cpus = os.environ.get("LLFE_RANK_CPUS")
    if rank_cpus and int(rank_cpus) > 0:
        return min(int(rank_cpus), 64)
    local = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1))
    return max(1, min(usable_cores() // local, 64))


def _pool(workers=None):
    global _POOL
    from concurrent.futures import ThreadPoolExecutor

    with _POOL_LOCK:
        want = workers or default_decode_threads()
        if _POOL is None or _POOL._max_workers != want:
            if _POOL is not None:
                _POOL.shutdown(wait=False)
            _POOL = ThreadPoolExecutor(max_workers=want, thread_name_prefix="llfe-decode")
        return _POOL


def decode_many(blobs, workers=None) -> list:
    """decode_bgr over a thread pool; returns arrays or DecodeError instances, in order."""

    def one(b):
        try:
            return decode_bgr(b)
        except DecodeError as e:
            return e

    return list(_pool(workers).map(one, blobs))


def decode_batch(blobs, out=None, workers=None) -> np.ndarray:
    """Decode equally sized images into one N x H x W x 3 BGR uint8 batch (``out`` if
    given, e.g. a pinned host tensor's numpy view).  Raises DecodeError naming the first
    image that fails or whose size differs from the first image's."""
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        raise DecodeError("empty batch")
    hw = _image_size(blobs[0])
    first = None if hw is not None else decode_bgr(blobs[0])
    h, w = hw if hw is not None else first.shape[:2]
    if out is None:
        out = np.empty((len(blobs), h, w, 3), np.uint8)
    if out.shape != (len(blobs), h, w, 3) or out.dtype != np.uint8 or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous {(len(blobs), h, w, 3)} uint8 array, got {out.shape} {out.dtype}")
    todo = list(range(len(blobs)))
    if hw is not None:  # PNG / JPEG batch: native decoders, Pillow for whatever they leave
        st = _native(blobs, h, w, out, workers or default_decode_threads())
        todo = [i for i, s_ in enumerate(st) if s_ != 0]
    else:
        out[0] = first
        todo = todo[1:]

    def one(i):
        try:
            im = decode_bgr(blobs[i])
        except DecodeError:
            return f"image {i}: Failed to decode image"
        if im.shape[:2] != (h, w):
            return f"image {i}: size {im.shape[1]}x{im.shape[0]} differs from {w}x{h}"
        out[i] = im
        return None

    errs = [e for e in _pool(workers).map(one, todo) if e] if todo else []
    if errs:
        raise DecodeError(errs[0])
    return out


# ------------------------------------------------------- JPEG reconstruction on the device
# The same decode split in two (DESIGN.md §3 "JPEG reconstruction on the device"): the host
# stops after the entropy half (llfe_jpeg_read_coefs_batch: libjpeg-turbo's
# jpeg_read_coefficients), the quantised coefficients cross PCIe, and llfe_jpeg_reconstruct
# (csrc/jpeg_images.hip) writes the BGR batch in device memory, bit for bit what decode_batch
# writes on the host.  Opt-in: nothing above calls it.
_STAGE_RING = 3  # staging buffers per (size, count): extraction of batch k + 1 beside batch k's copy
_RINGS = {}  # family ("coefs" / "bytes" / "png") -> {(n, stride): ring}
_STAGE_LOCK = _threading.Lock()


def _ring(family, n, stride, make_descs):
    """The next of _STAGE_RING staging buffers of ``family`` for n records of `stride` bytes:
    (numpy view, *make_descs(n), torch tensor or None).  Pinned when torch sees a GPU.  A family
    that holds more than four (n, stride) keys drops its other ones; families do not evict each
    other."""
    with _STAGE_LOCK:
        rings = _RINGS.setdefault(family, {})
        ring = rings.setdefault((n, stride), {"next": 0, "bufs": []})
        if len(rings) > 4:  # other batch shapes: drop their pinned memory
            for k in [k for k in rings if k != (n, stride)]:
                del rings[k]
        if len(ring["bufs"]) < _STAGE_RING:  # (filled in order, then handed out round robin)
            tensor = None
            try:
                import torch

                if torch.cuda.is_available():
                    tensor = torch.empty((n, stride), dtype=torch.uint8, pin_memory=True)
            except ImportError:  # pragma: no cover - C-only deployments
                pass
            arr = tensor.numpy() if tensor is not None else np.empty((n, stride), np.uint8)
            ring["bufs"].append((arr, *make_descs(n), tensor))
        buf = ring["bufs"][ring["next"] % _STAGE_RING]
        ring["next"] += 1
        return buf


def _batch_blobs(blobs, size=None):
    """-> (the blobs as bytes, h, w) of a batch of equally sized images: ``size``, else the first
    blob's header, else a decode of the first blob.  DecodeError for an empty batch."""
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        raise DecodeError("empty batch")
    hw = size or _image_size(blobs[0])
    if hw is None:
        hw = decode_bgr(blobs[0]).shape[:2]
    return blobs, hw[0], hw[1]


def _slot_bytes(slot_bytes, h, w) -> int:
    if slot_bytes is not None and (slot_bytes <= 0 or slot_bytes % 16):
        raise ValueError("slot_bytes must be a positive multiple of 16")
    return slot_bytes or coef_slot_bytes(h, w)


def _device(device):
    import torch

    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


def _out_tensor(device, n, h, w, out):
    """-> (torch device, ``out`` checked, or a new n x h x w x 3 uint8 tensor on it)."""
    import torch

    dev = _device(device)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    if tuple(out.shape) != (n, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous {(n, h, w, 3)} uint8 tensor on {dev}")
    return dev, out


def _to_device(st, buf, dev, whole=False):
    """A device copy of a staged batch's buffer ``buf`` (n x stride): the used part of each
    accepted record (a record fills what its file is long, not the bucket; a subsampled JPEG
    about half of a 4:4:4 slot), or with ``whole`` the buffer in one copy when more than three
    quarters of a record is used."""
    import torch

    used, stride = st.used_bytes, buf.shape[1]
    host = st.tensor if st.tensor is not None else torch.from_numpy(buf)
    d = torch.empty(tuple(buf.shape), dtype=torch.uint8, device=dev)
    if whole and 4 * used > 3 * stride:
        d.copy_(host, non_blocking=True)
    else:
        for i, rc in enumerate(st.status):
            if rc == 0:
                d[i, :used].copy_(host[i, :used], non_blocking=True)
    return d


class StagedCoefs:
    """One batch after its host half: ``slots`` (n x slot_stride uint8, pinned when a GPU is
    present), ``descs`` (the llfe_jpeg_desc array), ``status`` per image, the blobs (for the
    images handed back to the host decoders) and the batch geometry."""

    def __init__(self, blobs, h, w, slots, descs, status, tensor=None):
        self.blobs, self.h, self.w = blobs, h, w
        self.slots, self.descs, self.status, self.tensor = slots, descs, status, tensor

    @property
    def used_bytes(self) -> int:
        """Bytes from the start of a slot that any image of the batch occupies."""
        end = 0
        for d in self.descs:
            for c in range(d.n_comp):
                k = d.comp[c]
                end = max(end, k.coef_offset + k.blocks_w * k.blocks_h * 128, k.quant_offset + 128)
        return end


def coef_slot_bytes(h: int, w: int) -> int:
    """llfe_jpeg_coef_slot_bytes: the slot of any eligible h x w image (4:4:4 worst case)."""
    from . import _lib

    n = _lib.lib().llfe_jpeg_coef_slot_bytes(int(h), int(w))
    if n < 0:
        raise ValueError(f"no JPEG coefficient slot for {w}x{h}")
    return int(n)


def _read_coefs(blobs, h, w, slots, descs, threads) -> list:
    """llfe_jpeg_read_coefs_batch over all blobs into slots[i] / descs[i]; -> status list."""
    from . import _lib

    ptrs, sizes, status, keep = _blob_table(blobs)
    _lib.lib().llfe_jpeg_read_coefs_batch(ptrs, sizes, len(blobs), h, w, slots.ctypes.data, slots.strides[0], descs,
                                          status, int(threads))
    del keep
    return list(status)


def stage_coefs(blobs, workers=None, slot_bytes=None, size=None) -> StagedCoefs:
    """The host half of decode_batch_device: entropy-decode every eligible JPEG of a batch of
    equally sized images into the next staging buffer of a ring of three (so a producer thread
    may stage batch k + 1 while batch k is copied and reconstructed).  Host only.
    ``slot_bytes`` (a multiple of 16; default coef_slot_bytes(h, w), the 4:4:4 worst case)
    sizes a slot: a feed known to be 4:2:0 needs half, and an image that does not fit is
    handed back to the host decoders like any other.  ``size`` (h, w) names the batch's image
    size instead of reading it from the first blob (a part of a batch staged on its own)."""
    from . import _lib

    blobs, h, w = _batch_blobs(blobs, size)
    if h > 65535 or w > 65535:  # beyond JPEG: nothing to stage, the host decoders take every image
        return StagedCoefs(blobs, h, w, None, None, [-5] * len(blobs))
    slots, descs, tensor = _ring("coefs", len(blobs), _slot_bytes(slot_bytes, h, w),
                                 lambda n: ((_lib.LlfeJpegDesc * n)(),))
    status = _read_coefs(blobs, h, w, slots, descs, workers or default_decode_threads())
    return StagedCoefs(blobs, h, w, slots, descs, status, tensor)


def _host_fill(st, todo, workers):
    """decode_batch's treatment of the images in `todo` of a staged batch of any family (its
    blobs, h and w are read): the native host decoders, Pillow for what they leave;
    -> len(todo) x h x w x 3, or DecodeError naming the image."""
    h, w = st.h, st.w
    sub = [st.blobs[i] for i in todo]
    out = np.empty((len(sub), h, w, 3), np.uint8)
    rcs = _native(sub, h, w, out, workers or default_decode_threads())

    def one(k):
        i = todo[k]
        try:
            im = decode_bgr(sub[k])
        except DecodeError:
            return f"image {i}: Failed to decode image"
        if im.shape[:2] != (h, w):
            return f"image {i}: size {im.shape[1]}x{im.shape[0]} differs from {w}x{h}"
        out[k] = im
        return None

    left = [k for k, rc in enumerate(rcs) if rc != 0]
    errs = [e for e in _pool(workers).map(one, left) if e] if left else []
    if errs:
        raise DecodeError(errs[0])
    return out


def reconstruct_staged(st: StagedCoefs, device=0, workers=None, out=None):
    """The device half: copy the staged coefficients across and reconstruct on the current
    stream; images the coefficient path handed back are decoded on the host (as decode_batch
    does) and copied into their places.  -> (N, H, W, 3) uint8 tensor on the device."""
    import torch

    from .backend import Backend

    n, h, w = len(st.blobs), st.h, st.w
    dev, out = _out_tensor(device, n, h, w, out)
    todo = [i for i, rc in enumerate(st.status) if rc != 0]
    if len(todo) < n:
        with torch.cuda.device(dev):
            Backend.get(dev.index).jpeg_reconstruct(_to_device(st, st.slots, dev, whole=True), st.descs, h, w, out)
    if todo:
        fill = torch.from_numpy(_host_fill(st, todo, workers)).to(dev)
        out[torch.tensor(todo, device=dev)] = fill
    return out


# ------------------------------------------------- JPEG decode of a mixed-size batch on the device
# The coefficient path for images that each have their own size (DESIGN.md §3 "JPEG decode of a
# mixed-size batch"): llfe_jpeg_images_layout reads the headers and lays tight slots one behind the
# other, llfe_jpeg_read_coefs_images fills them, the staged prefix crosses PCIe in one copy and
# llfe_jpeg_reconstruct_images (csrc/jpeg_images.hip) writes every image in one launch into one
# packed tensor, each image at a multiple of 16 (the packing Backend.thumbnail_pil_images uses).
# Opt-in: nothing above calls it.
_STAGE_BYTES = 1 << 30  # one staging buffer at most (LLFE_JPEG_STAGE_BYTES): three ring buffers
# of it stay at what the same-size path pins for 512 x 1080p


class StagedImages:
    """A batch of images of any sizes after its host half: ``images`` (the llfe_jpeg_image
    records: size and slot of every image), ``descs`` (the llfe_jpeg_desc array), ``slots`` (1-d
    uint8, pinned when a GPU is present; its first ``used_bytes`` bytes hold the slots),
    ``layout_status`` / ``status`` per image (the header stage's, and the final one: the header
    stage's where that is not 0, else the extraction's) and the blobs (for the images handed back
    to the host decoders).  ``orientation``: per image, the EXIF orientation the reconstruction
    has to apply (2 .. 8 only for files staged with ``orient=True``, else 1); the records keep the
    coded size."""

    def __init__(self, blobs, images, descs, layout_status, status, slots, used_bytes, tensor=None, orientation=None):
        self.blobs, self.images, self.descs = blobs, images, descs
        self.layout_status, self.status = layout_status, status
        self.slots, self.used_bytes, self.tensor = slots, used_bytes, tensor
        self.orientation = [1] * len(blobs) if orientation is None else list(orientation)


def _stage_cap() -> int:
    import os

    env = os.environ.get("LLFE_JPEG_STAGE_BYTES")
    return int(env) if env and int(env) > 0 else _STAGE_BYTES


def _stage_bucket(nbytes: int) -> int:
    """The ring key of a staging buffer: a power of two from 4 KiB to 16 MiB, 16 MiB steps above,
    so like feeds reuse their pinned memory."""
    if nbytes <= 1 << 24:
        return max(4096, 1 << max(nbytes - 1, 0).bit_length())
    return (nbytes + (1 << 24) - 1) >> 24 << 24


def images_layout(blobs, workers=None, orient=False):
    """llfe_jpeg_images_layout: -> (the llfe_jpeg_image array, status list, total slot bytes).
    Host only, headers only; out_offset is left 0.  ``orient=True``
    (llfe_jpeg_images_layout_flags, LLFE_JPEG_ORIENT): JPEGs with an EXIF orientation 2 .. 8 are
    eligible too, and a fourth element follows: the orientation of every image (1 where it has
    none or is not taken); the records hold the coded size."""
    import ctypes as C

    from . import _lib

    n = len(blobs)
    images = (_lib.LlfeJpegImage * n)()
    total = C.c_int64(0)
    ptrs, sizes, status, keep = _blob_table(blobs)
    if not orient:
        _lib.lib().llfe_jpeg_images_layout(ptrs, sizes, n, images, C.byref(total), status,
                                           int(workers or default_decode_threads()))
        del keep
        return images, list(status), int(total.value)
    orientation = (C.c_uint8 * n)()
    _lib.lib().llfe_jpeg_images_layout_flags(ptrs, sizes, n, images, C.byref(total), status,
                                             int(workers or default_decode_threads()), orientation, _lib.JPEG_ORIENT)
    del keep
    return images, list(status), int(total.value), list(orientation)


def _stage_images(blobs, images, layout_status, workers, orientation=None) -> StagedImages:
    """llfe_jpeg_read_coefs_images of ``blobs`` into the next staging buffer of the ring, the
    slots of ``images`` (laid one behind the other here) in it.  ``orientation`` (the layout's,
    under ``orient=True``): files with an EXIF orientation are taken (LLFE_JPEG_ORIENT)."""
    from . import _lib

    n, total = len(blobs), 0
    for m in images:
        m.slot_offset = total
        total += m.slot_bytes
    slots, tensor = _ring("images", 1, _stage_bucket(total), lambda n: ())
    descs = (_lib.LlfeJpegDesc * n)()
    status = [-5] * n  # (LLFE_ERR_UNSUPPORTED: nothing staged)
    if total:
        ptrs, sizes, st, keep = _blob_table(blobs)
        _lib.lib().llfe_jpeg_read_coefs_images_flags(ptrs, sizes, n, images, slots.ctypes.data, total, descs, st,
                                                     int(workers or default_decode_threads()),
                                                     0 if orientation is None else _lib.JPEG_ORIENT)
        del keep
        status = list(st)
    status = [a if a != 0 else b for a, b in zip(layout_status, status)]
    return StagedImages(blobs, images, descs, list(layout_status), status, slots[0], total, tensor, orientation)


def stage_coefs_images(blobs, workers=None, orient=False) -> StagedImages:
    """The host half of decode_images_device for one staging buffer: the headers of every blob
    (images_layout), then the entropy decode of every eligible JPEG, whatever its size and
    sampling class, into tight slots in the next staging buffer of a ring of three, keyed by a
    bucket of the total bytes.  Host only.  An image this path does not take has a non-zero
    status and slot_bytes 0.  ``orient=True``: files with an EXIF orientation 2 .. 8 are staged
    too, byte for byte as the same file without EXIF, and ``orientation`` carries the value for
    the reconstruction."""
    blobs = [bytes(b) for b in blobs]
    images, layout_status, _, *orientation = images_layout(blobs, workers, orient)
    return _stage_images(blobs, images, layout_status, workers, orientation[0] if orient else None)


def _decode_or_error(b):
    try:
        return decode_bgr(b)
    except DecodeError as e:
        return e


class _Chunk:
    """What one chunk of decode_images_device holds after its staging: ``status`` per image
    (non-zero: the host decoders take it) and ``parts``, each (places in the chunk, llfe_jpeg_image
    records, llfe_jpeg_desc records, coefficients, orientations): a StagedImages whose used prefix
    has yet to cross, or a device tensor of slots; the orientations are None (all 1) or one per
    record."""

    def __init__(self, status, parts):
        self.status, self.parts = status, parts


def _host_chunk(st: StagedImages) -> _Chunk:
    return _Chunk(st.status, [(list(range(len(st.blobs))), st.images, st.descs, st, st.orientation)])


def _run_images(blobs, images, layout_status, chunks, first, device, workers, stage, orientation=None) -> list:
    """decode_images_device after the header stage: ``chunks`` (lists of image indices, in order,
    together all of them) are staged (``stage(idx)`` -> _Chunk) and reconstructed one after the
    other into one packed tensor; ``first`` is chunk 0 already staged.  ``orientation``: the
    layout's per image (None: all 1); the place of an image with 5 .. 8 is width x height."""
    import torch

    from .backend import Backend

    n = len(blobs)
    dev = _device(device)
    pool = _pool(workers)
    # what the host decoders take is known after the header stage and chunk 0's extraction; the
    # output is laid out once those are decoded: such an image has the decoded array's size, not
    # the header's (an EXIF orientation 5..8 swaps height and width)
    known = {i for i in range(n) if layout_status[i] != 0 or images[i].slot_bytes == 0}
    known |= {i for k, i in enumerate(chunks[0]) if first.status[k] != 0}
    order = sorted(known)
    host = dict(zip(order, pool.map(_decode_or_error, [blobs[i] for i in order])))
    shape, offset, total = [], [], 0
    for i in range(n):
        r = host.get(i)
        hw = (0, 0) if isinstance(r, Exception) else r.shape[:2] if r is not None else (images[i].height, images[i].width)
        if r is None and orientation is not None and orientation[i] >= 5:
            hw = hw[::-1]
        shape.append(hw)
        offset.append(total)
        total = (total + hw[0] * hw[1] * 3 + 15) & ~15
    packed = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)

    def place(i):
        return packed[offset[i]: offset[i] + shape[i][0] * shape[i][1] * 3].view(shape[i][0], shape[i][1], 3)

    out = [host[i] if isinstance(host.get(i), Exception) else place(i) for i in range(n)]
    for k, idx in enumerate(chunks):
        ch = first if k == 0 else stage(idx)
        for sub, recs, descs, coefs, orient in ch.parts:
            for m, j in zip(recs, sub):
                m.out_offset = offset[idx[j]]
            if not any(d.n_comp for d in descs):
                continue
            with torch.cuda.device(dev):
                if isinstance(coefs, StagedImages):  # the staged prefix in one copy: the slots are tight
                    st = coefs
                    src = st.tensor[0] if st.tensor is not None else torch.from_numpy(st.slots)
                    coefs = torch.empty(st.used_bytes, dtype=torch.uint8, device=dev)
                    coefs.copy_(src[:st.used_bytes], non_blocking=True)
                if orient is not None and all(o == 1 for o in orient):
                    orient = None
                Backend.get(dev.index).jpeg_reconstruct_images(coefs, recs, descs, packed, orient)
        # a later chunk's extraction handed an image back: its place is laid out by its header
        late = [i for j, i in enumerate(idx) if ch.status[j] != 0 and i not in known]
        for i, r in zip(late, pool.map(_decode_or_error, [blobs[i] for i in late])):
            if isinstance(r, Exception):
                out[i] = r
            elif r.shape[:2] == shape[i]:
                host[i] = r
            else:  # (no file does this: its own tensor)
                out[i] = torch.from_numpy(r).to(dev)
    for i, r in host.items():
        if not isinstance(r, Exception):
            out[i].copy_(torch.from_numpy(r))
    return out


def _sub_images(images, idx):
    """Copies of the llfe_jpeg_image records at the places ``idx``."""
    from . import _lib

    return (_lib.LlfeJpegImage * len(idx))(*[_lib.LlfeJpegImage.from_buffer_copy(images[i]) for i in idx])


def reconstruct_staged_images(st: StagedImages, device=0, workers=None) -> list:
    """The device half of a StagedImages: the staged coefficients across in one copy, one
    llfe_jpeg_reconstruct_images launch on the current stream, and for every image with a
    non-zero status decode_bgr on the decode pool, copied into its place.  -> a list in input
    order: H x W x 3 uint8 device tensors (views into one packed tensor, each starting at a
    multiple of 16), a DecodeError instance in the place of an image nothing decodes."""
    if not st.blobs:
        return []
    return _run_images(st.blobs, st.images, st.layout_status, [list(range(len(st.blobs)))], _host_chunk(st), device,
                       workers, None, st.orientation)


def decode_images_device(blobs, device=0, workers=None, entropy="host", restarts=False, orient="host") -> list:
    """decode_many with the JPEG reconstruction on the GPU, for images of any sizes: -> a list in
    input order of H x W x 3 BGR uint8 device tensors, the same bytes decode_bgr returns, each a
    view into one packed tensor and starting at a multiple of 16; a DecodeError instance stands
    in the place of an image that cannot be decoded at all (decode_many's convention).  Eligible
    JPEGs (what decode_batch_device takes) are entropy-decoded on ``workers`` host threads into
    tight slots and reconstructed by csrc/jpeg_images.hip in one launch; every other image (PNG,
    CMYK, EXIF-rotated, other samplings, truncated files) goes through decode_bgr on the decode
    pool and is copied into its place, with the size of the decoded array.  Staging is bounded
    (LLFE_JPEG_STAGE_BYTES, default 1 GiB): a batch above it is staged and reconstructed in
    chunks of whole images into the one packed tensor, and an image that alone exceeds it takes
    the host decoder.  The result feeds Backend.process_images, Backend.thumbnail_pil_images and
    MicroBatcher.submit unchanged.

    ``entropy="device"`` moves the entropy decode of baseline single-scan JPEGs (without restart
    markers, or with them under ``restarts=True``) to the device as well, chunk by chunk
    (stage_bytes_images, entropy_decode_staged_images: csrc/jpeg_huff.hip): the host parses the
    headers, the file bytes cross PCIe in one copy and the kernels fill a device tensor of the
    chunk's tight slots, so LLFE_JPEG_STAGE_BYTES then bounds coefficient bytes that live in
    device memory only.  What the device hands back takes the host coefficient path above, what
    that hands back decode_bgr; the result is the same bytes in every case.

    ``orient="device"`` keeps JPEGs with an EXIF orientation 2 .. 8 (a phone's portrait shot is a
    6 or an 8) on these routes instead of handing them to decode_bgr: they are staged as the same
    file without EXIF and the reconstruction stores every pixel where ImageOps.exif_transpose
    puts it, so the place of a 5 .. 8 image is width x height x 3.  The bytes are decode_bgr's.
    ``orient="host"`` is the route above."""
    if entropy not in ("host", "device"):
        raise ValueError('entropy must be "host" or "device"')
    if orient not in ("host", "device"):
        raise ValueError('orient must be "host" or "device"')
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        return []
    images, layout_status, _, *orientation = images_layout(blobs, workers, orient == "device")
    orientation = orientation[0] if orient == "device" else None
    cap, chunks, room = _stage_cap(), [[]], 0
    for i, m in enumerate(images):
        if m.slot_bytes > cap:
            m.slot_bytes = 0  # (the host decoder's)
        if chunks[-1] and room + m.slot_bytes > cap:
            chunks.append([])
            room = 0
        chunks[-1].append(i)
        room += m.slot_bytes

    def stage(idx):
        sub, status = [blobs[i] for i in idx], [layout_status[i] for i in idx]
        ori = None if orientation is None else [orientation[i] for i in idx]
        if entropy == "host":
            return _host_chunk(_stage_images(sub, _sub_images(images, idx), status, workers, ori))
        return _device_chunk(sub, _sub_images(images, idx), status, device, workers, restarts, ori)

    return _run_images(blobs, images, layout_status, chunks, stage(chunks[0]), device, workers, stage, orientation)


# ------------------------------------------------------------ JPEG entropy decode on the device
# The entropy half on the device too (DESIGN.md §3 "JPEG entropy decode on the device"): the host
# only parses the headers (llfe_jpeg_parse_batch), the file's scan bytes cross PCIe instead of
# its coefficients, and llfe_jpeg_entropy_decode (csrc/jpeg_huff.hip) writes the coefficient
# slots stage_coefs writes.  For baseline single-scan files without restart markers, or
# (restarts=True) with them; every other image, and every image whose scan shows an anomaly,
# takes the paths above.
class StagedBytes:
    """One batch after llfe_jpeg_parse_batch: ``records`` (n x record_stride uint8, pinned when
    a GPU is present), ``descs`` / ``scans`` (the llfe_jpeg_desc / llfe_jpeg_scan arrays),
    ``status`` per image, the blobs, the batch geometry and the slot stride the descriptors'
    offsets were laid out for."""

    def __init__(self, blobs, h, w, records, descs, scans, status, slot_bytes, tensor=None):
        self.blobs, self.h, self.w = blobs, h, w
        self.records, self.descs, self.scans, self.status = records, descs, scans, status
        self.slot_bytes, self.tensor = slot_bytes, tensor

    @property
    def used_bytes(self) -> int:
        """Bytes from the start of a record that any image of the batch occupies."""
        from . import _lib

        return max([_lib.JPEG_RECORD_HEADER + ((s.scan_bytes + 15) & ~15) + 16 for s in self.scans if s.blocks_in_mcu],
                   default=0)


def stage_bytes(blobs, workers=None, slot_bytes=None, restarts=False, size=None) -> StagedBytes:
    """The host half of decode_batch_device(entropy="device"): parse the headers of every
    eligible JPEG of a batch of equally sized images (llfe_jpeg_parse_batch: baseline Huffman,
    one interleaved scan, no restart markers, and what stage_coefs asks) and stage quantisation
    tables, decode tables and the scan's bytes in the next buffer of a ring of three.  Host
    only; no entropy decoding happens here.  The record stride is a power-of-two bucket of the
    longest blob, so batches of like files reuse their pinned buffers.  ``restarts=True``
    (llfe_jpeg_parse_batch_flags, LLFE_JPEG_PARSE_RESTARTS) also takes files with a restart
    interval: their scans are staged with the markers in them and the records carry the
    interval, which is all the device half needs to know.  ``size`` as in stage_coefs."""
    from . import _lib

    blobs, h, w = _batch_blobs(blobs, size)
    n = len(blobs)
    if h > 65535 or w > 65535:  # beyond JPEG: nothing to stage
        return StagedBytes(blobs, h, w, None, None, None, [-5] * n, 0)
    slot_bytes = _slot_bytes(slot_bytes, h, w)
    longest = max(len(b) for b in blobs)
    stride = _lib.JPEG_RECORD_HEADER + max(4096, 1 << (longest + 32).bit_length())
    records, descs, scans, tensor = _ring("bytes", n, stride,
                                          lambda n: ((_lib.LlfeJpegDesc * n)(), (_lib.LlfeJpegScan * n)()))
    ptrs, sizes, status, keep = _blob_table(blobs)
    _lib.lib().llfe_jpeg_parse_batch_flags(ptrs, sizes, n, h, w, records.ctypes.data, stride, slot_bytes, descs, scans,
                                           status, int(workers or default_decode_threads()),
                                           _lib.JPEG_PARSE_RESTARTS if restarts else 0)
    del keep
    return StagedBytes(blobs, h, w, records, descs, scans, list(status), slot_bytes, tensor)


def entropy_reference(sb: StagedBytes, one_piece=False):
    """llfe_jpeg_entropy_reference, the host twin of csrc/jpeg_huff.hip, over a StagedBytes:
    -> (n x slot_bytes uint8 slots, status list).  For tests and for debugging the kernels."""
    import ctypes as C

    from . import _lib

    n = len(sb.blobs)
    slots = np.zeros((n, sb.slot_bytes), np.uint8)
    status = (C.c_int32 * n)()
    rc = _lib.lib().llfe_jpeg_entropy_reference(sb.records.ctypes.data, sb.records.size, sb.scans, sb.descs, n, sb.h,
                                                sb.w, slots.ctypes.data, sb.slot_bytes, status, int(bool(one_piece)))
    if rc != 0:
        raise ValueError(f"llfe_jpeg_entropy_reference: {rc}")
    return slots, list(status)


def entropy_decode_staged(sb: StagedBytes, device=0):
    """The device half of the entropy decode: one H2D of the staged records, then
    llfe_jpeg_entropy_decode on the current stream.  -> (n x slot_bytes uint8 device tensor of
    coefficient slots, the descriptors of the images the device took (n_comp 0 for the others),
    the device's status list)."""
    import torch

    from . import _lib
    from .backend import Backend

    n = len(sb.blobs)
    dev = _device(device)
    with torch.cuda.device(dev):
        d_rec = _to_device(sb, sb.records, dev)
        d_slots = torch.empty((n, sb.slot_bytes), dtype=torch.uint8, device=dev)
        status = Backend.get(dev.index).jpeg_entropy_decode(d_rec, sb.scans, sb.descs, sb.h, sb.w, d_slots)
    descs = (_lib.LlfeJpegDesc * n).from_buffer_copy(sb.descs)
    for i, rc in enumerate(status):
        if rc != 0:
            descs[i].n_comp = 0
    return d_slots, descs, status


def decode_staged_bytes(sb: StagedBytes, device=0, workers=None, out=None):
    """The device half of decode_batch_device(entropy="device"): the staged records across, the
    entropy kernels, llfe_jpeg_reconstruct with the descriptors of the images that passed, and
    for the others the host coefficient path (stage_coefs / reconstruct_staged), which leaves
    what it cannot take to the host decoders.  -> (N, H, W, 3) uint8 tensor on the device."""
    import torch

    from .backend import Backend

    n, h, w = len(sb.blobs), sb.h, sb.w
    dev, out = _out_tensor(device, n, h, w, out)
    status = [-5] * n
    if any(rc == 0 for rc in sb.status):
        d_slots, descs, status = entropy_decode_staged(sb, dev)
        if any(rc == 0 for rc in status):
            with torch.cuda.device(dev):
                Backend.get(dev.index).jpeg_reconstruct(d_slots, descs, h, w, out)
    todo = [i for i, rc in enumerate(status) if rc != 0]
    if todo:  # the host coefficient path first, the host decoders for what that hands back
        sub = torch.empty((len(todo), h, w, 3), dtype=torch.uint8, device=dev)
        try:
            reconstruct_staged(stage_coefs([sb.blobs[i] for i in todo], workers, size=(h, w)), dev, workers, sub)
        except DecodeError as e:
            raise _renumber(e, todo) from None
        out[torch.tensor(todo, device=dev)] = sub
    return out


# ------------------------------------------- JPEG entropy decode of a mixed-size batch on the device
# The two paths above joined (DESIGN.md §3 "JPEG entropy decode of a mixed-size batch"): the
# headers give tight slots (llfe_jpeg_images_layout) and records as long as their files
# (llfe_jpeg_records_layout), llfe_jpeg_parse_images stages the records one behind the other, the
# used prefix crosses PCIe in one copy and llfe_jpeg_entropy_decode_images (csrc/jpeg_huff.hip)
# fills the tight slots llfe_jpeg_reconstruct_images reads.
class StagedByteImages:
    """A batch of images of any sizes after llfe_jpeg_parse_images: ``images`` (the llfe_jpeg_image
    records: size and tight slot of every image), ``descs`` / ``scans`` (the llfe_jpeg_desc /
    llfe_jpeg_scan arrays), ``records`` (1-d uint8, pinned when a GPU is present; its first
    ``used_bytes`` bytes hold the records), ``slot_bytes`` (the bytes of all slots),
    ``layout_status`` / ``status`` per image (the header stage's, and the final one), the
    blobs and ``orientation`` (as StagedImages')."""

    def __init__(self, blobs, images, descs, scans, layout_status, status, records, used_bytes, slot_bytes, tensor=None,
                 orientation=None):
        self.blobs, self.images, self.descs, self.scans = blobs, images, descs, scans
        self.layout_status, self.status = layout_status, status
        self.records, self.used_bytes, self.slot_bytes, self.tensor = records, used_bytes, slot_bytes, tensor
        self.orientation = [1] * len(blobs) if orientation is None else list(orientation)


def _stage_bytes_images(blobs, images, layout_status, workers, restarts, orientation=None) -> StagedByteImages:
    """llfe_jpeg_parse_images of ``blobs`` into the next staging buffer of the ring, the slots of
    ``images`` and the records (llfe_jpeg_records_layout) laid one behind the other here.
    ``orientation`` as in _stage_images."""
    import ctypes as C

    from . import _lib

    n, total = len(blobs), 0
    for m in images:
        m.slot_offset = total
        total += m.slot_bytes
    ptrs, sizes, st, keep = _blob_table(blobs)
    offsets, used = (C.c_int64 * n)(), C.c_int64(0)
    _lib.lib().llfe_jpeg_records_layout(sizes, images, n, offsets, C.byref(used))
    records, tensor = _ring("byte_images", 1, _stage_bucket(used.value), lambda n: ())
    descs, scans = (_lib.LlfeJpegDesc * n)(), (_lib.LlfeJpegScan * n)()
    status = [-5] * n  # (LLFE_ERR_UNSUPPORTED: nothing staged)
    if used.value:
        _lib.lib().llfe_jpeg_parse_images(ptrs, sizes, n, images, offsets, records.ctypes.data, used.value, descs, scans,
                                          st, int(workers or default_decode_threads()),
                                          (_lib.JPEG_PARSE_RESTARTS if restarts else 0) |
                                          (0 if orientation is None else _lib.JPEG_ORIENT))
        status = list(st)
    del keep
    status = [a if a != 0 else b for a, b in zip(layout_status, status)]
    return StagedByteImages(blobs, images, descs, scans, list(layout_status), status, records[0], int(used.value), total,
                            tensor, orientation)


def stage_bytes_images(blobs, workers=None, restarts=False, orient=False) -> StagedByteImages:
    """The host half of decode_images_device(entropy="device") for one staging buffer: the headers
    of every blob (images_layout), then llfe_jpeg_parse_images: quantisation tables, decode tables
    and the scan's bytes of every eligible JPEG (what stage_bytes takes), whatever its size and
    sampling class, one record behind the other in the next staging buffer of a ring of three,
    keyed by a bucket of the total bytes.  Host only; no entropy decoding happens here.  An image
    this path does not take has a non-zero status, n_comp 0 and blocks_in_mcu 0.  ``restarts`` as
    in stage_bytes, ``orient`` as in stage_coefs_images."""
    blobs = [bytes(b) for b in blobs]
    images, layout_status, _, *orientation = images_layout(blobs, workers, orient)
    return _stage_bytes_images(blobs, images, layout_status, workers, restarts, orientation[0] if orient else None)


def entropy_reference_images(st: StagedByteImages, one_piece=False):
    """llfe_jpeg_entropy_reference_images, the host twin of csrc/jpeg_huff.hip over tight slots:
    -> (1-d uint8 array of st.slot_bytes, status list).  For tests and for debugging the kernels."""
    import ctypes as C

    from . import _lib

    n = len(st.blobs)
    slots = np.zeros(max(st.slot_bytes, 1), np.uint8)
    status = (C.c_int32 * n)()
    rc = _lib.lib().llfe_jpeg_entropy_reference_images(st.records.ctypes.data, st.used_bytes, st.scans, st.descs, st.images,
                                                       n, slots.ctypes.data, st.slot_bytes, status, int(bool(one_piece)))
    if rc != 0:
        raise ValueError(f"llfe_jpeg_entropy_reference_images: {rc}")
    return slots[:st.slot_bytes], list(status)


def entropy_decode_staged_images(st: StagedByteImages, device=0, slots=None):
    """The device half of the entropy decode of images of any sizes: one H2D of the used prefix
    of the staged records, then llfe_jpeg_entropy_decode_images on the current stream into
    ``slots`` (a 1-d uint8 device tensor of at least st.slot_bytes; allocated when None).
    -> (the coefficient tensor, the descriptors of the images the device took (n_comp 0 for the
    others), the device's status list)."""
    import torch

    from . import _lib
    from .backend import Backend

    n = len(st.blobs)
    dev = _device(device)
    with torch.cuda.device(dev):
        src = st.tensor[0] if st.tensor is not None else torch.from_numpy(st.records)
        d_rec = torch.empty(max(st.used_bytes, 1), dtype=torch.uint8, device=dev)
        d_rec[:st.used_bytes].copy_(src[:st.used_bytes], non_blocking=True)
        if slots is None:
            slots = torch.empty(max(st.slot_bytes, 1), dtype=torch.uint8, device=dev)
        status = Backend.get(dev.index).jpeg_entropy_decode_images(d_rec[:st.used_bytes], st.scans, st.descs, st.images,
                                                                   slots)
    descs = (_lib.LlfeJpegDesc * n).from_buffer_copy(st.descs)
    for i, rc in enumerate(status):
        if rc != 0:
            descs[i].n_comp = 0
    return slots, descs, status


def _device_chunk(blobs, images, layout_status, device, workers, restarts, orientation=None) -> _Chunk:
    """One chunk of decode_images_device(entropy="device"): parse, copy, entropy kernels; the
    images the device hands back go through the host coefficient path (_stage_images)."""
    n = len(blobs)
    sb = _stage_bytes_images(blobs, images, layout_status, workers, restarts, orientation)
    status, parts = [-5] * n, []
    if any(rc == 0 for rc in sb.status):
        d_slots, descs, status = entropy_decode_staged_images(sb, device)
        parts.append((list(range(n)), sb.images, descs, d_slots, orientation))
    todo = [j for j, rc in enumerate(status) if rc != 0]
    status = list(status)
    if todo:
        st = _stage_images([blobs[j] for j in todo], _sub_images(images, todo), [layout_status[j] for j in todo], workers,
                           None if orientation is None else [orientation[j] for j in todo])
        parts.append((todo, st.images, st.descs, st, st.orientation))
        for j, rc in zip(todo, st.status):
            status[j] = rc
    return _Chunk(status, parts)


# ------------------------------------------------------------------ PNG decode on the device
# PNG the same way (DESIGN.md §3 "PNG decode on the device"): the host only walks the chunks
# (llfe_png_parse_batch), the file's deflate stream crosses PCIe instead of its pixels, and
# llfe_png_decode_device (csrc/png_inflate.hip) inflates, unfilters and converts.  For 8-bit RGB /
# RGBA files that are not interlaced; every other image, and every image whose stream shows an
# anomaly, goes through the host decoders as in decode_batch.
class StagedPng:
    """One batch after llfe_png_parse_batch: ``records`` (n x record_stride uint8, pinned when a
    GPU is present), ``descs`` (the llfe_png_desc array), ``status`` per image, the blobs and the
    batch geometry."""

    def __init__(self, blobs, h, w, records, descs, status, tensor=None):
        self.blobs, self.h, self.w = blobs, h, w
        self.records, self.descs, self.status, self.tensor = records, descs, status, tensor

    @property
    def used_bytes(self) -> int:
        """Bytes from the start of a record that any image of the batch occupies."""
        return max([((d.deflate_bytes + 15) & ~15) + 32 for d in self.descs if d.deflate_bytes], default=0)

    @property
    def raw_stride(self) -> int:
        """Bytes per image of inflated rows (a multiple of 16) that hold any image of the batch."""
        return max(16, (max([d.raw_bytes for d in self.descs], default=0) + 15) & ~15)


def stage_png(blobs, workers=None, size=None) -> StagedPng:
    """The host half of decode_batch_device(png="device"): walk the chunks of every eligible PNG
    of a batch of equally sized images (llfe_png_parse_batch: 8-bit RGB or RGBA, not interlaced)
    and stage its deflate stream in the next buffer of a ring of three.  Host only; nothing is
    inflated here.  The record stride is a bucket of the longest blob (a power of two up to
    1 MiB, 1 MiB steps above), so batches of like files reuse their pinned buffers.  ``size`` (h, w) names the batch's image size
    instead of reading it from the first blob (a part of a batch staged on its own)."""
    from . import _lib

    blobs, h, w = _batch_blobs(blobs, size)
    n = len(blobs)
    longest = max(len(b) for b in blobs)
    stride = max(4096, 1 << (longest + 64).bit_length())
    if stride > 1 << 20:  # (above 1 MiB a power of two wastes pinned memory: 1 MiB steps)
        stride = (longest + 64 + (1 << 20) - 1) >> 20 << 20
    records, descs, tensor = _ring("png", n, stride, lambda n: ((_lib.LlfePngDesc * n)(),))
    ptrs, sizes, status, keep = _blob_table(blobs)
    _lib.lib().llfe_png_parse_batch(ptrs, sizes, n, h, w, records.ctypes.data, stride, descs, status,
                                    int(workers or default_decode_threads()))
    del keep
    return StagedPng(blobs, h, w, records, descs, list(status), tensor)


def png_reference(sp: StagedPng):
    """llfe_png_decode_reference, the host twin of csrc/png_inflate.hip, over a StagedPng:
    -> (n x raw_stride uint8 inflated rows, n x h x w x 3 BGR, status list).  Both arrays start
    as zeros.  For tests and for debugging the kernels."""
    import ctypes as C

    from . import _lib

    n = len(sp.blobs)
    raw = np.zeros((n, sp.raw_stride), np.uint8)
    out = np.zeros((n, sp.h, sp.w, 3), np.uint8)
    status = (C.c_int32 * n)()
    rc = _lib.lib().llfe_png_decode_reference(sp.records.ctypes.data, sp.records.size, sp.descs, n, sp.h, sp.w,
                                              raw.ctypes.data, raw.shape[1], out.ctypes.data, status)
    if rc != 0:
        raise ValueError(f"llfe_png_decode_reference: {rc}")
    return raw, out, list(status)


def png_decode_staged(sp: StagedPng, device=0, out=None, raw=None):
    """The device half without the fallback: one H2D of the used part of each staged record, then
    llfe_png_decode_device on the current stream into ``out`` (allocated when None; the places of
    the images with a non-zero status are undefined).  -> (out, the device's status list)."""
    import torch

    from .backend import Backend

    n, h, w = len(sp.blobs), sp.h, sp.w
    dev = _device(device)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        d_rec = _to_device(sp, sp.records, dev)
        if raw is None:
            raw = torch.empty((n, sp.raw_stride), dtype=torch.uint8, device=dev)
        status = Backend.get(dev.index).png_decode(d_rec, sp.descs, h, w, out, raw)
    return out, status


def decode_staged_png(sp: StagedPng, device=0, workers=None, out=None):
    """The device half of decode_batch_device(png="device"): the staged records across, the
    kernels, and for every image with a non-zero parse or device status decode_batch's own
    treatment (the native host decoders, Pillow for what they leave), so errors read as
    decode_batch's.  -> (N, H, W, 3) uint8 tensor on the device."""
    import torch

    n, h, w = len(sp.blobs), sp.h, sp.w
    dev, out = _out_tensor(device, n, h, w, out)
    status = list(sp.status)
    if any(rc == 0 for rc in sp.status):
        status = png_decode_staged(sp, dev, out)[1]
    todo = [i for i, rc in enumerate(status) if rc != 0]
    if todo:
        fill = torch.from_numpy(_host_fill(sp, todo, workers)).to(dev)
        out[torch.tensor(todo, device=dev)] = fill
    return out


def _is_png(b) -> bool:
    return b[:8] == _PNG_SIG


def _renumber(e, index):
    """A DecodeError of a part of a batch, naming the image by its place in the whole batch."""
    head, sep, tail = str(e).partition(":")
    k = head[len("image "):]
    return DecodeError(f"image {index[int(k)]}:{tail}" if sep and head.startswith("image ") and k.isdigit() else str(e))


def decode_batch_device(blobs, device=0, workers=None, out=None, entropy="host", restarts=False, png="host"):
    """decode_batch with the reconstruction on the GPU: equally sized images -> one
    (N, H, W, 3) BGR uint8 tensor on ``device``, the same bytes decode_batch returns.  Eligible
    JPEGs (8-bit greyscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0, EXIF orientation 1, no decoder
    warning) are entropy-decoded on ``workers`` host threads and reconstructed by
    csrc/jpeg_images.hip; everything else (PNG, CMYK, EXIF-rotated, other samplings, truncated
    files) goes through the host decoders image by image.  Raises DecodeError as decode_batch
    does.  The result feeds Backend.process / submit unchanged.

    ``entropy="device"`` moves the entropy decode of baseline single-scan JPEGs without restart
    markers to the device as well (csrc/jpeg_huff.hip): the file bytes cross PCIe, not the
    coefficients.  Images it does not take, and images whose scan the kernels find anomalous,
    go through the ``entropy="host"`` path; the result is the same bytes in every case.
    ``restarts=True`` lets it take files with restart intervals too (stage_bytes).

    ``png="device"`` sends the PNGs of the batch down a device path of their own (stage_png /
    decode_staged_png: csrc/png_inflate.hip inflates, unfilters and converts 8-bit RGB / RGBA
    files), the other images down the path ``entropy`` names, all into the one tensor; with
    ``png="host"`` PNGs go through the host decoders as before."""
    if entropy not in ("host", "device"):
        raise ValueError('entropy must be "host" or "device"')
    if png not in ("host", "device"):
        raise ValueError('png must be "host" or "device"')
    if png == "device":
        blobs = [bytes(b) for b in blobs]
        pngs = [i for i, b in enumerate(blobs) if _is_png(b)]
        if pngs:
            return _decode_split(blobs, pngs, device, workers, out, entropy, restarts)
    if entropy == "host":
        return reconstruct_staged(stage_coefs(blobs, workers), device, workers, out)
    return decode_staged_bytes(stage_bytes(blobs, workers, restarts=restarts), device, workers, out)


def _decode_split(blobs, pngs, device, workers, out, entropy, restarts):
    """decode_batch_device(png="device") of a batch that holds PNGs (at the places `pngs`): the
    batch split by signature, each part down its path with the batch's size, the results
    gathered into one tensor.  Of the parts' errors the one naming the first image is raised,
    as decode_batch would."""
    import torch

    blobs, h, w = _batch_blobs(blobs)
    n = len(blobs)
    dev, out = _out_tensor(device, n, h, w, out)

    def png_part(sub, o):
        return decode_staged_png(stage_png(sub, workers, size=(h, w)), dev, workers, o)

    def other_part(sub, o):
        if entropy == "host":
            return reconstruct_staged(stage_coefs(sub, workers, size=(h, w)), dev, workers, o)
        return decode_staged_bytes(stage_bytes(sub, workers, restarts=restarts, size=(h, w)), dev, workers, o)

    if len(pngs) == n:
        return png_part(blobs, out)
    is_png = set(pngs)
    errs = []
    for index, part in ((pngs, png_part), ([i for i in range(n) if i not in is_png], other_part)):
        sub = torch.empty((len(index), h, w, 3), dtype=torch.uint8, device=dev)
        try:
            part([blobs[i] for i in index], sub)
        except DecodeError as e:
            errs.append(_renumber(e, index))
            continue
        out[torch.tensor(index, device=dev)] = sub
    if errs:
        def place(e):
            k = str(e).partition(":")[0][len("image "):]
            return int(k) if k.isdigit() else -1

        raise min(errs, key=place)
    return out
