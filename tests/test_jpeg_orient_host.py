"""EXIF orientation in the host half of the mixed-size JPEG decode (LLFE_JPEG_ORIENT), CPU only:
the orientation map's CPU twin (llfe_jpeg_orient_reference) against the table restated with NumPy,
the layout with and without the flag, staging that equals the staging of the same pixels saved
without EXIF byte for byte, the flag refused by the same-size parser, and the composition that
pins the parity bar: the twin applied to decode_bgr of the plain file is decode_bgr of the
oriented file."""
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib, decode
from tests import jpeg_orient_cases as OC

OK, INVALID, UNSUPPORTED = 0, _lib.LLFE_ERR_INVALID, -5
CLASSES = [dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(gray=True)]


def _reference(src, o):
    """llfe_jpeg_orient_reference into a buffer pre-filled with 0xA5: -> (rc, flat result)."""
    h, w = src.shape[:2]
    dst = np.full(h * w * 3, 0xA5, np.uint8)
    src = np.ascontiguousarray(src)
    return _lib.lib().llfe_jpeg_orient_reference(src.ctypes.data, h, w, o, dst.ctypes.data), dst


def _blob(arr, o, gray=False, **kw):
    return OC.jpeg(arr[:, :, 1].copy() if gray else arr, o, **kw)


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (7, 1), (5, 12), (37, 53)])
def test_reference_equals_the_table(hw):
    h, w = hw
    src = OC.pixels(h, w, 100 * h + w)
    for o in OC.ORIENTATIONS:
        rc, dst = _reference(src, o)
        want = OC.reindex(src, o)
        assert rc == OK and want.shape == ((w, h, 3) if o >= 5 else (h, w, 3))
        assert np.array_equal(dst.reshape(want.shape), want), o
    for o in (0, 9, -1, 256 + 6):
        rc, dst = _reference(src, o)
        assert rc == INVALID and bool((dst == 0xA5).all()), o
    lib = _lib.lib()
    assert lib.llfe_jpeg_orient_reference(None, 1, 1, 1, src.ctypes.data) == INVALID
    assert lib.llfe_jpeg_orient_reference(src.ctypes.data, 1, 1, 1, None) == INVALID
    assert lib.llfe_jpeg_orient_reference(src.ctypes.data, 0, 1, 1, src.ctypes.data) == INVALID


def _layout(blobs, flags, with_array=True):
    n = len(blobs)
    images = (_lib.LlfeJpegImage * n)()
    total = C.c_int64(-1)
    orientation = (C.c_uint8 * n)(*([0xEE] * n))
    ptrs, sizes, status, keep = decode._blob_table(blobs)
    rc = _lib.lib().llfe_jpeg_images_layout_flags(ptrs, sizes, n, images, C.byref(total), status, 2,
                                                  orientation if with_array else None, flags)
    return rc, images, list(status), total.value, list(orientation)


def test_layout_with_and_without_the_flag():
    arr = OC.pixels(24, 40, 5)
    blobs = [_blob(arr, o, **CLASSES[o % 4]) for o in range(2, 9)]
    plain = [_blob(arr, None, **CLASSES[o % 4]) for o in range(2, 9)]
    rc, images, status, total, orientation = _layout(blobs, _lib.JPEG_ORIENT)
    assert rc == OK and status == [OK] * 7 and orientation == list(range(2, 9))
    assert [(m.height, m.width) for m in images] == [(24, 40)] * 7  # the coded size, also for 5 .. 8
    # the slots of the same pixels without EXIF
    _, p_images, p_status, p_total, p_orientation = _layout(plain, _lib.JPEG_ORIENT)
    assert p_status == [OK] * 7 and p_orientation == [1] * 7 and p_total == total
    assert [(m.slot_offset, m.slot_bytes) for m in images] == [(m.slot_offset, m.slot_bytes) for m in p_images]
    # without the flag: refused as before, by the old entry point and by flags = 0
    n_images, n_status, _ = decode.images_layout(blobs)
    assert n_status == [UNSUPPORTED] * 7 and all(m.slot_bytes == 0 for m in n_images)
    rc, images, status, total, orientation = _layout(blobs, 0)
    assert rc == UNSUPPORTED and status == [UNSUPPORTED] * 7 and total == 0 and orientation == [1] * 7
    assert _layout(blobs, 0, with_array=False)[2] == [UNSUPPORTED] * 7
    # the flag needs the array; no other bit is a flag
    assert _layout(blobs, _lib.JPEG_ORIENT, with_array=False)[0] == INVALID
    for bad in (1, 2, 0x80, _lib.JPEG_ORIENT | 1):
        assert _layout(blobs, bad)[0] == INVALID, bad
    # the Python wrapper
    images, status, total, orientation = decode.images_layout(blobs, orient=True)
    assert status == [OK] * 7 and orientation == list(range(2, 9))


def test_layout_still_refuses_what_is_not_a_rotation():
    arr = OC.pixels(20, 30, 6)
    cmyk = OC.jpeg(np.random.default_rng(7).integers(0, 256, (20, 30, 4), dtype=np.uint8), 6)
    blobs = [cmyk, _blob(arr, 9), _blob(arr, 0), _blob(arr, 6), _blob(arr, 1), b"\xff\xd8\xffjunk"]
    rc, images, status, total, orientation = _layout(blobs, _lib.JPEG_ORIENT)
    assert status[:3] == [UNSUPPORTED] * 3 and status[3:5] == [OK, OK] and status[5] != OK
    assert orientation == [1, 1, 1, 6, 1, 1]
    assert [m.slot_bytes for m in images[:3]] == [0] * 3 and images[5].slot_bytes == 0
    st = decode.stage_coefs_images(blobs, workers=2, orient=True)
    assert [rc == OK for rc in st.status] == [False, False, False, True, True, False]
    sb = decode.stage_bytes_images(blobs, workers=2, orient=True)
    assert [rc == OK for rc in sb.status] == [False, False, False, True, True, False]


@pytest.mark.parametrize("cls", range(4))
def test_staging_equals_the_plain_file(cls):
    """Slots, descriptors and records of an oriented file are those of the same pixels saved
    without EXIF; without the option the file is handed back as before."""
    arr = OC.pixels(37, 53, 40 + cls)
    kw = CLASSES[cls]
    oriented = [_blob(arr, o, quality=80, **kw) for o in OC.ORIENTATIONS]
    plain = [_blob(arr, None, quality=80, **kw)] * 8
    a, b = decode.stage_coefs_images(oriented, workers=2, orient=True), decode.stage_coefs_images(plain, workers=2)
    assert a.status == b.status == [OK] * 8 and a.orientation == list(OC.ORIENTATIONS) and b.orientation == [1] * 8
    assert a.used_bytes == b.used_bytes > 0
    assert np.array_equal(a.slots[:a.used_bytes], b.slots[:b.used_bytes])
    assert bytes(a.descs) == bytes(b.descs) and bytes(a.images) == bytes(b.images)
    assert (a.images[5].height, a.images[5].width) == (37, 53)
    off = decode.stage_coefs_images(oriented, workers=2)
    assert off.status == [OK] + [UNSUPPORTED] * 7 and off.orientation == [1] * 8
    # the records of the device entropy decode: tables and scan bytes, one image at a time (a
    # record's room follows its file's length, which the EXIF segment changes)
    for o in OC.ORIENTATIONS:
        ra = decode.stage_bytes_images([oriented[o - 1]], workers=1, orient=True)
        rb = decode.stage_bytes_images([plain[0]], workers=1)
        assert ra.status == rb.status == [OK] and ra.orientation == [o]
        assert bytes(ra.descs) == bytes(rb.descs) and bytes(ra.scans) == bytes(rb.scans)
        used = _lib.JPEG_RECORD_HEADER + ((ra.scans[0].scan_bytes + 15) & ~15) + 16
        assert 0 < used <= min(ra.used_bytes, rb.used_bytes)
        assert np.array_equal(ra.records[:used], rb.records[:used])
        # and the twin of the kernels decodes them into the slot of the coefficient path
        slots, status = decode.entropy_reference_images(ra)
        assert status == [OK] and np.array_equal(slots, a.slots[a.images[o - 1].slot_offset:][:slots.size])
    assert decode.stage_bytes_images(oriented, workers=2).status == [OK] + [UNSUPPORTED] * 7


def test_flag_refused_by_the_same_size_entry_points():
    b = _blob(OC.pixels(16, 16, 3), 6)
    ptrs, sizes, status, keep = decode._blob_table([b])
    stride = _lib.JPEG_RECORD_HEADER + 4096
    rec = np.full(stride, 0xA5, np.uint8)
    descs, scans = (_lib.LlfeJpegDesc * 1)(), (_lib.LlfeJpegScan * 1)()
    for flags in (_lib.JPEG_ORIENT, _lib.JPEG_ORIENT | _lib.JPEG_PARSE_RESTARTS):
        rc = _lib.lib().llfe_jpeg_parse_batch_flags(ptrs, sizes, 1, 16, 16, rec.ctypes.data, stride,
                                                    decode.coef_slot_bytes(16, 16), descs, scans, status, 1, flags)
        assert rc == INVALID and bool((rec == 0xA5).all())
    # the mixed-size entry points take the bit and no other new one
    images, _, total, _ = decode.images_layout([b], orient=True)
    slots = np.zeros(total, np.uint8)
    read = lambda flags: _lib.lib().llfe_jpeg_read_coefs_images_flags(ptrs, sizes, 1, images, slots.ctypes.data, total,
                                                                      descs, status, 1, flags)
    assert read(_lib.JPEG_ORIENT) == OK and read(0) == UNSUPPORTED and read(1) == INVALID and read(8) == INVALID
    # the same-size staging hands an oriented file back as before
    assert decode.stage_coefs([b], workers=1).status == [UNSUPPORTED]
    assert decode.stage_bytes([b], workers=1).status == [UNSUPPORTED]


@pytest.mark.parametrize("cls", range(4))
def test_composition_is_decode_bgr(cls):
    """decode_bgr of a file with orientation o is decode_bgr of the same file without EXIF
    through the map: the bar of the device route, pinned without a GPU."""
    for h, w in ((1, 1), (37, 53), (5, 300)):
        arr = OC.pixels(h, w, 7 * h + w + cls)
        plain = decode.decode_bgr(_blob(arr, None, quality=85, **CLASSES[cls]))
        assert plain.shape == (h, w, 3)
        for o in OC.ORIENTATIONS:
            want = decode.decode_bgr(_blob(arr, o, quality=85, **CLASSES[cls]))
            rc, got = _reference(plain, o)
            assert rc == OK and np.array_equal(got.reshape(want.shape), want), (h, w, o)


def test_option_values():
    from low_level_feature_extraction_amd.image_processor import ImageProcessor

    with pytest.raises(ValueError, match="orient must be"):
        decode.decode_images_device([b"x"], orient="gpu")
    with pytest.raises(ValueError, match="orient must be"):
        ImageProcessor.auto_process_images([b"x"], orient="gpu")
    with pytest.raises(ValueError, match='orient="device" needs decode="device"'):
        ImageProcessor.auto_process_images([b"x"], device=True, orient="device")
