"""Drop-in validate_and_preprocess_image (app/services/analyze/utils.py:90-152).

Decode on the host (cv2.imdecode IMREAD_COLOR semantics, decode.py), then the
mode-dependent downscale of utils.py:118-143:

    none          -> no resize
    auto          -> INTER_AREA     when max(h, w) > 2000
    high_quality  -> INTER_LANCZOS4 when max(h, w) > 4000
    performance   -> INTER_LINEAR   when max(h, w) > 1000

with new_size = (int(w * s), int(h * s)), s = max_dim / max(h, w) (the size rule is
llfe_preprocess_size in the C ABI).  The resize itself runs on the GPU
(llfe_resize_cv: OpenCV's fixed-point / area tables, csrc/cvresize.hip).  No BASELINE
configuration triggers a resize (1920 < 2000, 3840 < 4000).
"""
from __future__ import annotations

import logging
from enum import Enum

import numpy as np

from .decode import DecodeError, decode_bgr

logger = logging.getLogger(__name__)

_LIMITS = {"auto": (2000, "INTER_AREA"), "high_quality": (4000, "INTER_LANCZOS4"),
           "performance": (1000, "INTER_LINEAR")}


class PreprocessingMode(str, Enum):
    NONE = "none"
    AUTO = "auto"
    HIGH_QUALITY = "high_quality"
    PERFORMANCE = "performance"


_CODE = {"INTER_LINEAR": 1, "INTER_AREA": 3, "INTER_LANCZOS4": 4}


def preprocess_size(w: int, h: int, preprocessing: str):
    """-> (new_w, new_h, interpolation name) or None (utils.py:118-143)."""
    from . import backend

    plan = backend.preprocess_size(w, h, preprocessing)
    if plan is None:
        return None
    return plan[0], plan[1], _LIMITS[preprocessing][1]


def preprocess_decoded(image: np.ndarray, preprocessing: str, device: int = 0) -> np.ndarray:
    """The mode resize of utils.py:118-143 on a decoded BGR image (GPU; the HIP
    extension must be present -- there is no CPU fallback)."""
    h, w = image.shape[:2]
    plan = preprocess_size(w, h, preprocessing)
    if plan is None:
        return image
    from .backend import Backend

    out = Backend.get(device).resize_cv(image, plan[0], plan[1], _CODE[plan[2]])
    return out.cpu().numpy()


def _http_exception(status_code: int, detail: str):
    try:
        from fastapi import HTTPException

        return HTTPException(status_code=status_code, detail=detail)
    except ImportError:  # pragma: no cover - fastapi absent
        return ValueError(detail)


_DECODE_DETAIL = "Failed to decode image. The file may be corrupted or in an unsupported format."


def validate_and_preprocess_images(images_bytes, preprocessing: str, device: bool = False, decode: str = "host",
                                   entropy: str = "host", restarts: bool = False, orient: str = "host") -> list:
    """Batched validate_and_preprocess_image: decode, then the mode resize of every image the
    rule resizes, whatever the sizes, in one llfe_preprocess_images call
    (Backend.preprocess_images).  Returns the images in input order; an input that fails to
    decode gets the exception validate_and_preprocess_image would raise, in its place.

    ``device=False``: host arrays with the bytes of ``preprocess_decoded`` (the results of the
    one call come back in one device-to-host copy; an image the rule leaves is the decoded array
    itself).  ``device=True``: device tensors (views into one packed tensor), which run_batch,
    Backend.process_images and MicroBatcher.submit take as they are.

    ``decode`` / ``entropy`` / ``restarts`` / ``orient`` are those of
    ImageProcessor.auto_process_images: ``decode="device"`` (with ``device=True`` only) chains
    decode.decode_images_device, so a JPEG's pixels never cross PCIe."""
    from .backend import Backend
    from .decode import decode_images_device, decode_many

    if decode not in ("host", "device"):
        raise ValueError('decode must be "host" or "device"')
    if decode == "device" and not device:
        raise ValueError('decode="device" needs device=True')
    if entropy not in ("host", "device"):
        raise ValueError('entropy must be "host" or "device"')
    if entropy == "device" and decode != "device":
        raise ValueError('entropy="device" needs decode="device"')
    if restarts and entropy != "device":
        raise ValueError('restarts=True needs entropy="device"')
    if orient not in ("host", "device"):
        raise ValueError('orient must be "host" or "device"')
    if orient == "device" and decode != "device":
        raise ValueError('orient="device" needs decode="device"')
    preprocessing = getattr(preprocessing, "value", preprocessing)
    mode = preprocessing if preprocessing in _LIMITS else "none"  # (other names do not resize)
    if decode == "device":
        decoded = decode_images_device(list(images_bytes), Backend.get().device, entropy=entropy, restarts=restarts,
                                       orient=orient)
    else:
        decoded = decode_many(list(images_bytes))
    out: list = list(decoded)
    for i, im in enumerate(decoded):
        if isinstance(im, Exception):
            inner = _http_exception(400, _DECODE_DETAIL)
            out[i] = _http_exception(400, f"Image validation or preprocessing failed: {str(inner)}")
    good = [i for i, im in enumerate(decoded) if not isinstance(im, Exception)]
    if not device:  # only what the rule resizes goes to the device
        good = [i for i in good if preprocess_size(decoded[i].shape[1], decoded[i].shape[0], mode)]
    if good:
        res = Backend.get().preprocess_images([decoded[i] for i in good], mode, host=not device)
        for i, t in zip(good, res):
            out[i] = t
    return out


async def validate_and_preprocess_image(image_bytes: bytes, request_id: str, preprocessing: str) -> np.ndarray:
    try:
        try:
            image = decode_bgr(image_bytes)
        except DecodeError:
            raise _http_exception(400, "Failed to decode image. The file may be corrupted or in an unsupported format.")
        return preprocess_decoded(image, preprocessing)
    except Exception as e:
        logger.error(f"Error in validate_and_preprocess_image: {str(e)}", exc_info=True)
        raise _http_exception(400, f"Image validation or preprocessing failed: {str(e)}")
