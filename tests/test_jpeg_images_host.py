"""The host half of the JPEG decode of a mixed-size batch (llfe_jpeg_images_layout and
llfe_jpeg_read_coefs_images behind decode.stage_coefs_images), CPU only: the layout of a shuffled
batch of every case of tests/jpeg_restate.py, the statuses of what the path hands back, staging
that equals the per-image staging of decode.stage_coefs byte for byte, the NumPy restatement on
the ragged staging against the host decoder, slots that are too small or out of range, the
argument checks, the tiling query and the record size."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode, synth
from tests import jpeg_restate as R

OK, INVALID, CAPACITY, UNSUPPORTED = 0, _lib.LLFE_ERR_INVALID, -3, -5
MCU = {R.GRAY: (8, 8), R.S444: (8, 8), R.S422: (16, 8), R.S420: (16, 16)}  # width x height


def _up16(v):
    return (v + 15) & ~15


@pytest.fixture(scope="module")
def batch():
    """Every case in a fixed shuffled order: (cases, blobs, the staged batch, each blob staged
    alone by decode.stage_coefs: (used bytes, descriptor bytes, a copy of the used part of its
    slot); copies, because stage_coefs hands its staging buffers out again)."""
    order = np.random.default_rng(2024).permutation(len(R.CASES))
    cases = [R.CASES[i] for i in order]
    blobs = [R.blob(*c) for c in cases]
    alone = []
    for b in blobs:
        one = decode.stage_coefs([b], workers=1)
        assert one.status == [0]
        alone.append((one.used_bytes, bytes(one.descs[0]), one.slots[0, :_up16(one.used_bytes)].copy()))
    return cases, blobs, decode.stage_coefs_images(blobs, workers=3), alone


def _call_layout(blobs, threads=2):
    n = len(blobs)
    images = (_lib.LlfeJpegImage * max(n, 1))()
    for m in images:
        m.out_offset = 4242
    total = C.c_int64(-1)
    ptrs, sizes, status, keep = decode._blob_table(blobs)
    rc = _lib.lib().llfe_jpeg_images_layout(ptrs, sizes, n, images, C.byref(total), status, threads)
    return rc, images, list(status), total.value


def test_layout_of_a_shuffled_batch(batch):
    cases, blobs, st, alone = batch
    rc, images, status, total = _call_layout(blobs)
    assert rc == OK and status == [OK] * len(blobs)
    off = 0
    for i, b in enumerate(blobs):
        m = images[i]
        assert (m.height, m.width) == decode._image_size(b) == cases[i][:2]
        assert m.slot_bytes == _up16(alone[i][0]) and m.slot_bytes % 16 == 0
        assert m.slot_offset == off and m.slot_offset % 16 == 0
        assert m.out_offset == 4242  # the caller's
        off += m.slot_bytes
    assert total == off
    # a 4:2:0 file takes half a 4:4:4 slot
    big = {c[2]: images[i].slot_bytes for i, c in enumerate(cases) if c[:2] == (240, 321)}
    assert big[0] < 0.51 * big[2]


def test_layout_statuses():
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    ex = Image.Exif()
    ex[0x0112] = 6
    rot = io.BytesIO()
    Image.fromarray(arr).save(rot, "JPEG", exif=ex.tobytes())
    cmyk = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (20, 30, 4), dtype=np.uint8), "CMYK").save(cmyk, "JPEG")
    blobs = [synth.encode_png(arr[:18, :26].copy()), rot.getvalue(), cmyk.getvalue(), b"\x01\x02\x03\x04garb", b"",
             R.blob(17, 33, 0)]
    rc, images, status, total = _call_layout(blobs)
    assert rc == UNSUPPORTED  # the first non-OK status
    assert status == [UNSUPPORTED] * 5 + [OK]
    assert [(m.height, m.width) for m in images] == [(18, 26), (24, 40), (20, 30), (0, 0), (0, 0), (17, 33)]
    assert [m.slot_bytes for m in images[:5]] == [0] * 5 and images[5].slot_offset == 0
    assert total == images[5].slot_bytes > 0
    # corrupt data (a JPEG signature, then nothing libjpeg can read) is INVALID, 0 x 0
    rc, images, status, total = _call_layout([b"\xff\xd8\xff\xe0" + b"\x00" * 30])
    assert (rc, status, total) == (INVALID, [INVALID], 0) and (images[0].height, images[0].width) == (0, 0)


def test_staging_equals_per_image_staging(batch):
    cases, blobs, st, alone = batch
    assert st.layout_status == [OK] * len(blobs) and st.status == [OK] * len(blobs)
    assert st.used_bytes == sum(m.slot_bytes for m in st.images) <= st.slots.size
    for i in range(len(blobs)):
        m = st.images[i]
        assert bytes(st.descs[i]) == alone[i][1], cases[i]
        assert np.array_equal(st.slots[m.slot_offset: m.slot_offset + m.slot_bytes], alone[i][2]), cases[i]


def test_restatement_on_the_ragged_staging_equals_decode_bgr(batch):
    cases, blobs, st, _ = batch
    for i, b in enumerate(blobs):
        m = st.images[i]
        one = decode.StagedCoefs([b], m.height, m.width, st.slots[None, m.slot_offset: m.slot_offset + m.slot_bytes],
                                 (_lib.LlfeJpegDesc * 1)(st.descs[i]), [0])
        assert np.array_equal(R.restate(one), decode.decode_bgr(b)), cases[i]


def _read(blobs, images, slots, total, threads=2):
    n = len(blobs)
    descs = (_lib.LlfeJpegDesc * max(n, 1))()
    ptrs, sizes, status, keep = decode._blob_table(blobs)
    rc = _lib.lib().llfe_jpeg_read_coefs_images(ptrs, sizes, n, images, slots.ctypes.data, total, descs, status, threads)
    return rc, descs, list(status)


def test_slot_too_small_and_slot_out_of_range():
    blobs = [R.blob(37, 53, 2), R.blob(17, 33, 0), R.blob(16, 16, 11), R.blob(37, 53, 0)]
    _, images, status, total = _call_layout(blobs)
    assert status == [OK] * 4
    good = np.full(total, 0xAB, np.uint8)
    rc, _, status = _read(blobs, images, good, total)
    assert rc == OK and status == [OK] * 4
    # 16 bytes short: handed back, the neighbours' slots as before, its own not written
    images[1].slot_bytes -= 16
    slots = np.full(total, 0xAB, np.uint8)
    rc, descs, status = _read(blobs, images, slots, total)
    assert rc == UNSUPPORTED and status == [OK, UNSUPPORTED, OK, OK] and descs[1].n_comp == 0
    lo, hi = images[1].slot_offset, images[2].slot_offset
    assert np.array_equal(slots[:lo], good[:lo]) and np.array_equal(slots[hi:], good[hi:])
    assert bool((slots[lo:hi] == 0xAB).all())
    # another size than the record says
    images[1].slot_bytes += 16
    images[2].height += 1
    rc, descs, status = _read(blobs, images, slots, total)
    assert status == [OK, OK, CAPACITY, OK] and descs[2].n_comp == 0
    images[2].height -= 1
    # nothing staged
    images[0].slot_bytes = 0
    rc, descs, status = _read(blobs, images, slots, total)
    assert status == [UNSUPPORTED, OK, OK, OK] and descs[0].n_comp == 0
    _, images, _, _ = _call_layout(blobs)
    # a slot past slots_bytes: refused as a whole, nothing written
    for edit in (lambda m: setattr(m[3], "slot_offset", m[3].slot_offset + 16), lambda m: setattr(m[0], "slot_offset", -16),
                 lambda m: setattr(m[2], "slot_offset", m[2].slot_offset + 8), lambda m: setattr(m[1], "slot_bytes", total + 16)):
        _, bad, _, _ = _call_layout(blobs)
        edit(bad)
        slots = np.full(total, 0xAB, np.uint8)
        rc, descs, status = _read(blobs, bad, slots, total)
        assert rc == INVALID and status == [0] * 4 and bool((slots == 0xAB).all())
        assert all(d.n_comp == 0 for d in descs)


def test_argument_checks():
    lib = _lib.lib()
    blobs = [R.blob(8, 8, 0)]
    ptrs, sizes, status, keep = decode._blob_table(blobs)
    images = (_lib.LlfeJpegImage * 1)()
    descs = (_lib.LlfeJpegDesc * 1)()
    total = C.c_int64(7)
    slots = np.zeros(4096, np.uint8)
    assert lib.llfe_jpeg_reconstruct_images(None, None, 0, images, descs, 1, None, 0, None) == INVALID
    assert lib.llfe_jpeg_images_layout(ptrs, sizes, -1, images, C.byref(total), status, 1) == INVALID
    assert lib.llfe_jpeg_images_layout(ptrs, sizes, 1, None, C.byref(total), status, 1) == INVALID
    assert lib.llfe_jpeg_images_layout(ptrs, sizes, 1, images, None, status, 1) == INVALID
    assert lib.llfe_jpeg_images_layout(ptrs, sizes, 1, images, C.byref(total), None, 1) == INVALID
    assert lib.llfe_jpeg_images_layout(None, None, 0, None, C.byref(total), None, 1) == OK and total.value == 0
    assert lib.llfe_jpeg_images_layout(ptrs, sizes, 1, images, C.byref(total), status, 0) == OK and total.value == 768
    assert lib.llfe_jpeg_read_coefs_images(ptrs, sizes, -1, images, slots.ctypes.data, 4096, descs, status, 1) == INVALID
    assert lib.llfe_jpeg_read_coefs_images(ptrs, sizes, 1, images, None, 4096, descs, status, 1) == INVALID
    assert lib.llfe_jpeg_read_coefs_images(ptrs, sizes, 1, images, slots.ctypes.data, 4096, None, status, 1) == INVALID
    assert lib.llfe_jpeg_read_coefs_images(ptrs, sizes, 1, images, slots.ctypes.data, 4096, descs, None, 1) == INVALID
    assert lib.llfe_jpeg_read_coefs_images(ptrs, sizes, 1, images, slots.ctypes.data, -1, descs, status, 1) == INVALID
    assert lib.llfe_jpeg_read_coefs_images(None, None, 0, None, None, 0, None, None, 1) == OK
    assert lib.llfe_jpeg_read_coefs_images(ptrs, sizes, 1, images, slots.ctypes.data, 4096, descs, status, 1) == OK
    assert descs[0].n_comp == 3 and descs[0].sampling == R.S420
    # a NULL blob
    null = (C.c_void_p * 1)(None)
    assert lib.llfe_jpeg_images_layout(null, sizes, 1, images, C.byref(total), status, 1) == INVALID and status[0] == INVALID


def test_tiling_query():
    lib = _lib.lib()
    for cls, (mw, mh) in MCU.items():
        tw, th = C.c_int32(0), C.c_int32(0)
        assert lib.llfe_jpeg_images_tiling(cls, C.byref(tw), C.byref(th)) == OK
        assert tw.value > 0 and th.value > 0 and tw.value % mw == 0 and th.value % mh == 0
    tw, th = C.c_int32(0), C.c_int32(0)
    for cls in (0, 5, -1, 9):
        assert lib.llfe_jpeg_images_tiling(cls, C.byref(tw), C.byref(th)) == INVALID
    assert lib.llfe_jpeg_images_tiling(R.S420, None, C.byref(th)) == INVALID


def test_record_size_and_abi(tmp_path):
    import os
    import subprocess

    assert C.sizeof(_lib.LlfeJpegImage) == 32
    assert _lib.lib().llfe_abi_version() == 3
    # the header's layout, through the compiler
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in _lib.LlfeJpegImage._fields_]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "llfe.h"\nint main(void){\n'
                   'printf("%zu", sizeof(llfe_jpeg_image));\n'
                   + "".join(f'printf(" %zu", offsetof(llfe_jpeg_image, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32] + [getattr(_lib.LlfeJpegImage, f).offset for f in fields]


def test_stage_bucket_and_empty_batch():
    assert decode._stage_bucket(0) == 4096 and decode._stage_bucket(4097) == 8192
    assert decode._stage_bucket(1 << 24) == 1 << 24 and decode._stage_bucket((1 << 24) + 1) == 2 << 24
    st = decode.stage_coefs_images([b"junk", b""])
    assert st.status == [UNSUPPORTED, UNSUPPORTED] and st.used_bytes == 0
    assert decode.decode_images_device([]) == []
    from low_level_feature_extraction_amd.image_processor import ImageProcessor

    with pytest.raises(ValueError):
        ImageProcessor.auto_process_images([], decode="device")
    with pytest.raises(ValueError):
        ImageProcessor.auto_process_images([], device=True, decode="gpu")
