"""The host half of the split JPEG decode (llfe_jpeg_read_coefs_batch, csrc/jpeg_decode.cpp)
and the arithmetic of the device half, CPU only.

For every case the NumPy restatement (tests/jpeg_restate.py) of libjpeg-turbo's
reconstruction -- dequantise, ISLOW inverse DCT, fancy upsampling, YCbCr -> BGR -- applied to
the extracted coefficients must equal the native host decoder's bytes
(cv2.imdecode(IMREAD_COLOR), utils.py:108-109, image_processor.py:208-211).  That pins the
hand-declared jpeg_component_info / JQUANT_TBL / jpeg_memory_mgr layouts and the arithmetic
that csrc/jpeg_recon_core.h restates against the installed library without a GPU.
"""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode, synth
from tests import jpeg_restate as R

UNSUPPORTED, INVALID, CAPACITY = -5, -1, -3


def _read(blobs, h, w, fill=0xA5, threads=1):
    """-> (status list, slots, descs) with the slots pre-filled, so a write shows."""
    stride = decode.coef_slot_bytes(h, w)
    slots = np.full((len(blobs), stride), fill, np.uint8)
    descs = (_lib.LlfeJpegDesc * len(blobs))()
    return decode._read_coefs(blobs, h, w, slots, descs, threads), slots, descs


_STATS = {}


@pytest.mark.parametrize("h,w,k", R.CASES)
def test_restatement_of_coefficients_equals_host_decode(h, w, k):
    b = R.blob(h, w, k)
    rc, want = R.host_decode(b)
    assert rc == 0
    st = decode.stage_coefs([b], workers=1)
    assert st.status == [0]
    d = st.descs[0]
    kw = R.SETTINGS[k]
    cls = R.GRAY if kw.get("gray") else {0: R.S444, 1: R.S422, 2: R.S420}[kw["subsampling"]]
    assert (d.n_comp, d.sampling) == (1 if cls == R.GRAY else 3, cls)
    got = R.restate(st, 0, _STATS)
    assert np.array_equal(got, want)
    # the slot size is the bound of every extent the descriptor names
    assert st.used_bytes <= decode.coef_slot_bytes(h, w) == st.slots.shape[1]
    hs, vs = (2 if cls in (R.S422, R.S420) else 1), (2 if cls == R.S420 else 1)
    for c in range(d.n_comp):
        q = d.comp[c]
        assert (q.width, q.height) == ((-(-w // hs), -(-h // vs)) if c else (w, h))
        assert (q.blocks_w, q.blocks_h) == (-(-q.width // 8), -(-q.height // 8))
        assert q.coef_offset % 16 == 0 and q.quant_offset % 16 == 0


def test_inputs_leave_the_sample_range_before_limiting():
    """The case list exercises the IDCT's limiting and the colour clamps (counted by the
    restatement while the cases above ran; computed here when this test runs alone)."""
    if not _STATS:
        for h, w, k in R.CASES:
            if R.SETTINGS[k]["quality"] == 1:
                R.restate(decode.stage_coefs([R.blob(h, w, k)], workers=1), 0, _STATS)
    assert _STATS["idct_out_of_range"] >= 1 and _STATS["colour_out_of_range"] >= 1


@pytest.mark.parametrize("k", [2, 6, 13])
def test_samples_far_outside_the_range_saturate_as_the_library_does(k):
    """Quality-100 noise with its all-ones tables scaled by 5: samples land more than 384
    outside 0..255, where libjpeg-turbo's C code (a 1024-entry table under a 10-bit mask)
    wraps and its SIMD code saturates.  The installed library decides; jpeg_images.hip and
    the restatement saturate."""
    b = R.scaled_tables(R.blob(16, 16, k), 5)
    rc, want = R.host_decode(b)
    st = decode.stage_coefs([b], workers=1)
    assert rc == 0 and st.status == [0]
    stats = {}
    assert np.array_equal(R.restate(st, 0, stats), want)
    assert stats["idct_out_of_range"] > 0
    assert not np.array_equal(R.restate(st, 0, limit="mask"), want)


@pytest.mark.parametrize("factor", [12, 40, 255])
@pytest.mark.parametrize("h,w,k", [(16, 16, 2), (37, 53, 6), (37, 53, 13), (16, 16, 3)])
def test_hand_made_tables_decode_as_the_library_decodes_them(h, w, k, factor):
    """Tables scaled until the dequantised values leave what any encoder emits: the library's
    SIMD code then wraps its 16-bit products and sums and saturates its 16-bit workspace.  The
    restatement (and jpeg_images.hip, test_gpu_jpeg_recon.py) follows it bit for bit, so such
    files too decode to the host path's bytes."""
    b = R.scaled_tables(R.blob(h, w, k), factor)
    rc, want = R.host_decode(b)
    st = decode.stage_coefs([b], workers=1)
    assert rc == 0 and st.status == [0]
    assert np.array_equal(R.restate(st, 0), want)


def test_batch_statuses_threads_and_untouched_slots():
    h, w = 20, 30
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ok = R.jpeg(arr, quality=80)
    cmyk = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "CMYK").save(cmyk, "JPEG")
    ex = Image.Exif()
    ex[0x0112] = 6
    exif6 = io.BytesIO()
    Image.fromarray(arr).save(exif6, "JPEG", exif=ex.tobytes())
    ex[0x0112] = 1
    exif1 = io.BytesIO()
    Image.fromarray(arr).save(exif1, "JPEG", exif=ex.tobytes())
    big = R.jpeg(rng.integers(0, 256, (64, 96, 3), dtype=np.uint8), quality=90)
    truncated = big[:len(big) // 2] + b"\xff\xd9"
    bad = bytearray(ok)
    sof = bytes(bad).index(b"\xff\xc0")
    bad[sof + 7:sof + 9] = b"\x00\x00"  # SOF0 width 0: libjpeg's error_exit
    png = synth.encode_png(arr)
    other_size = R.jpeg(arr[:10], quality=80)
    blobs = [ok, cmyk.getvalue(), exif6.getvalue(), exif1.getvalue(), bytes(bad), png, other_size, ok]
    want = [0, UNSUPPORTED, UNSUPPORTED, 0, INVALID, UNSUPPORTED, CAPACITY, 0]
    for threads in (1, 3):
        st, slots, descs = _read(blobs, h, w, threads=threads)
        assert st == want
        for i, rc in enumerate(st):
            if rc:
                assert (slots[i] == 0xA5).all() and descs[i].n_comp == 0
            else:
                assert descs[i].n_comp == 3 and not (slots[i] == 0xA5).all()
        assert np.array_equal(slots[0], slots[7])
    # a truncated scan is a libjpeg warning: the host path fills the missing rows, this path
    # hands the image back
    st, slots, descs = _read([truncated], 64, 96)
    assert st == [UNSUPPORTED] and (slots == 0xA5).all() and descs[0].n_comp == 0
    assert R.host_decode(truncated)[0] == 0
    # the return value is the first non-OK status
    n = len(blobs)
    ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in blobs])
    sizes = (C.c_uint64 * n)(*[len(b) for b in blobs])
    status = (C.c_int32 * n)()
    stride = decode.coef_slot_bytes(h, w)
    slots = np.zeros((n, stride), np.uint8)
    descs = (_lib.LlfeJpegDesc * n)()
    L = _lib.lib()
    assert L.llfe_jpeg_read_coefs_batch(ptrs, sizes, n, h, w, slots.ctypes.data, stride, descs, status, 2) == UNSUPPORTED
    assert L.llfe_jpeg_read_coefs_batch(ptrs, sizes, 1, h, w, slots.ctypes.data, stride, descs, status, 2) == 0
    assert L.llfe_jpeg_read_coefs_batch(ptrs, sizes, 1, 0, w, slots.ctypes.data, stride, descs, status, 2) == INVALID


def test_slot_bytes():
    assert decode.coef_slot_bytes(1, 1) == 384 + 3 * 128
    assert decode.coef_slot_bytes(1080, 1920) == 384 + 3 * 135 * 240 * 128
    assert decode.coef_slot_bytes(17, 33) % 128 == 0
    L = _lib.lib()
    assert L.llfe_jpeg_coef_slot_bytes(0, 5) < 0 and L.llfe_jpeg_coef_slot_bytes(5, 65536) < 0
    assert C.sizeof(_lib.LlfeJpegDesc) == 104


def test_desc_layout_matches_header_via_compiler(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "llfe.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(llfe_jpeg_desc), offsetof(llfe_jpeg_desc, sampling),'
                   'offsetof(llfe_jpeg_desc, comp), offsetof(llfe_jpeg_desc, comp[1].height),'
                   'offsetof(llfe_jpeg_desc, comp[2].coef_offset), offsetof(llfe_jpeg_desc, comp[2].quant_offset));'
                   'return 0;}')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, K = _lib.LlfeJpegDesc, _lib.LlfeJpegComp
    assert got == [C.sizeof(D), D.sampling.offset, D.comp.offset, D.comp.offset + C.sizeof(K) + K.height.offset,
                   D.comp.offset + 2 * C.sizeof(K) + K.coef_offset.offset,
                   D.comp.offset + 2 * C.sizeof(K) + K.quant_offset.offset]


def test_stage_coefs_ring_and_mixed_batch_statuses():
    imgs = [synth.synth_numpy(i, 40, 56, seed=4) for i in range(3)]
    blobs = [R.jpeg(imgs[0][:, :, ::-1].copy(), quality=90), synth.encode_png(imgs[1]),
             R.jpeg(imgs[2][:, :, 1].copy(), quality=70)]
    seen = []
    for _ in range(4):
        st = decode.stage_coefs(blobs, workers=2)
        assert st.status == [0, UNSUPPORTED, 0] and (st.h, st.w) == (40, 56)
        assert [d.n_comp for d in st.descs] == [3, 0, 1]
        for i in (0, 2):
            assert np.array_equal(R.restate(st, i), R.host_decode(blobs[i])[1])
        seen.append(st.slots.ctypes.data)
    assert len(set(seen[:3])) == 3 and seen[3] == seen[0]  # a ring of three staging buffers
