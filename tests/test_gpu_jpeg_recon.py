"""JPEG reconstruction on the device (llfe_jpeg_reconstruct, the tile kernel of
csrc/jpeg_images.hip, behind decode.decode_batch_device): the same bytes as the host decoder
(decode.decode_batch, i.e. cv2.imdecode(IMREAD_COLOR) at utils.py:108-109 /
image_processor.py:208-211), for every case of tests/jpeg_restate.py (which test_jpeg_coefs.py
pins against the installed libjpeg-turbo on the CPU), for mixed batches with host fallbacks,
and on the kernel's seams: the tile of each sampling class (64 x 32 for 4:4:4, 128 x 32 for
4:2:2 and grey, 128 x 64 for 4:2:0) in both directions, rows and images that are / are not
4-byte aligned, classes mixed in one call, an image in the middle of a call that is not
staged.  A descriptor that points outside its slot is refused by the host check before any
launch."""
import dataclasses
import io

import numpy as np
import pytest
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode, synth
from tests import jpeg_restate as R

pytestmark = pytest.mark.gpu


def _same(blobs, **kw):
    want = decode.decode_batch(blobs, workers=2)
    got = decode.decode_batch_device(blobs, workers=2, **kw)
    assert tuple(got.shape) == want.shape and got.is_cuda
    got = got.cpu().numpy()
    for i in range(len(blobs)):
        assert np.array_equal(got[i], want[i]), f"image {i} differs at {np.argwhere(got[i] != want[i])[:4].tolist()}"
    return got


@pytest.mark.parametrize("h,w", R.SIZES)
def test_case_list_equals_host_decode(backend, h, w):
    """Every setting (4:4:4 / 4:2:2 / 4:2:0 / grey, quality 1..100, progressive, optimised,
    restart intervals) at one size per call."""
    blobs = [R.blob(h, w, k) for k in range(len(R.SETTINGS))]
    st = decode.stage_coefs(blobs, workers=2)
    assert st.status == [0] * len(blobs)  # all reconstructed on the device, none by the fallback
    _same(blobs)


def test_mixed_batch_with_fallbacks(backend):
    h, w = 72, 100
    imgs = [synth.synth_numpy(i, h, w, seed=9) for i in range(12)]
    rgb = [im[:, :, ::-1].copy() for im in imgs]
    ex = Image.Exif()
    ex[0x0112] = 3  # rotate 180: the same size after exif_transpose
    rot = io.BytesIO()
    Image.fromarray(rgb[10]).save(rot, "JPEG", exif=ex.tobytes())
    blobs = [R.jpeg(rgb[0], quality=90, subsampling=0), R.jpeg(rgb[1], quality=80, subsampling=1),
             R.jpeg(rgb[2], quality=70, subsampling=2), R.jpeg(rgb[3][:, :, 1].copy(), quality=85),
             R.jpeg(rgb[4], quality=88, progressive=True), synth.encode_png(imgs[5]),
             R.jpeg(rgb[6], quality=30, subsampling=2, optimize=True), R.jpeg(rgb[7], quality=95, subsampling=1),
             R.jpeg(rgb[8], quality=75, restart_marker_blocks=2), synth.encode_png(imgs[9]), rot.getvalue(),
             R.jpeg(rgb[11], quality=1, subsampling=0)]
    st = decode.stage_coefs(blobs, workers=3)
    assert [rc != 0 for rc in st.status] == [i in (5, 9, 10) for i in range(12)]
    got = _same(blobs)
    assert np.array_equal(got[5], imgs[5]) and np.array_equal(got[9], imgs[9])
    assert np.array_equal(got[10], decode.decode_bgr(blobs[10]))


@pytest.mark.parametrize("h,w,sub", [(70, 530, 2), (9, 260, 2), (12, 256, 1), (5, 1028, 0), (130, 136, 2),
                                     (40, 72, 0), (40, 136, 1)])
def test_kernel_seams(backend, h, w, sub):
    """Sizes across the tile of the class, which one workgroup reconstructs: several tiles in a
    row with 4-byte aligned rows (dword stores) and without (byte tail), a last tile of a few
    columns or rows, 2 x 2 tiles of the 4:4:4 tile (40 x 72) and of the 4:2:2 and grey tile
    (40 x 136), 3 x 2 of the 4:2:0 tile (130 x 136: chroma halo blocks on every side); a
    subsampled batch fills half a slot, so its slots are copied piecewise."""
    rng = np.random.default_rng(h * w)
    blobs = [R.jpeg(synth.synth_numpy(0, h, w, seed=2)[:, :, ::-1].copy(), quality=85, subsampling=sub),
             R.jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), quality=40, subsampling=sub),
             R.jpeg(rng.integers(0, 256, (h, w), dtype=np.uint8), quality=90)]
    _same(blobs)


def test_hand_made_tables_equal_host_decode(backend):
    """Quantisation tables scaled by 5 (samples far outside 0..255: saturation), 40 and 255
    (16-bit products and sums wrap in the library's SIMD code, the whole-block DC shortcut
    differs from the full pass): still the host decoder's bytes."""
    blobs = [R.scaled_tables(R.blob(37, 53, k), f) for k in (2, 6, 13, 3) for f in (5, 40, 255)]
    assert decode.stage_coefs(blobs, workers=2).status == [0] * len(blobs)
    _same(blobs)


def test_three_classes_in_one_call(backend):
    """Five 40 x 56 images of three sampling classes in one call: every image's tiles find
    their own record, slot and place in the result."""
    rng = np.random.default_rng(11)
    blobs = [R.jpeg(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), quality=50 + 10 * i, subsampling=i % 3)
             for i in range(5)]
    _same(blobs)


def test_out_tensor_and_process_equal_host_path(backend):
    import torch

    imgs = [synth.synth_numpy(i, 128, 160, seed=21) for i in range(4)]
    blobs = [R.jpeg(im[:, :, ::-1].copy(), quality=85, subsampling=(2, 1, 0, 2)[i]) for i, im in enumerate(imgs)]
    out = torch.zeros((4, 128, 160, 3), dtype=torch.uint8, device="cuda:0")
    dev = decode.decode_batch_device(blobs, out=out)
    assert dev.data_ptr() == out.data_ptr()
    host = decode.decode_batch(blobs)
    feats = ("colors", "shapes", "shadows")
    a = backend.process(dev, feats, seed=5)
    b = backend.process(host, feats, seed=5)
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        for f in dataclasses.fields(x):
            u, v = getattr(x, f.name), getattr(y, f.name)
            assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v, f.name


@pytest.mark.parametrize("h,w", [(17, 33), (16, 16)])
def test_skipped_image_in_the_middle(backend, h, w):
    """One image per sampling class, the second not staged (n_comp = 0): its place in out
    stays as it was and the images behind it still land at their own index.  17 x 33 is 1683
    bytes per image, so every later image starts at an odd address and takes byte stores;
    16 x 16 is 768 bytes per image, dword stores."""
    import torch

    rng = np.random.default_rng(h * w)
    blobs = [R.jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), quality=80, subsampling=sub) for sub in (2, 1, 0)]
    blobs.append(R.jpeg(rng.integers(0, 256, (h, w), dtype=np.uint8), quality=80))
    st = decode.stage_coefs(blobs, workers=2)
    assert st.status == [0, 0, 0, 0]
    descs = (_lib.LlfeJpegDesc * 4).from_buffer_copy(st.descs)
    descs[1].n_comp = 0
    out = torch.full((4, h, w, 3), 77, dtype=torch.uint8, device="cuda:0")
    backend.jpeg_reconstruct(torch.from_numpy(st.slots).cuda(), descs, h, w, out=out)
    got = out.cpu().numpy()
    want = decode.decode_batch(blobs, workers=2)
    assert (got[1] == 77).all()
    for i in (0, 2, 3):
        assert np.array_equal(got[i], want[i]), f"image {i} differs at {np.argwhere(got[i] != want[i])[:4].tolist()}"


def test_descriptor_outside_the_slot_is_refused_on_the_host(backend):
    import torch

    blobs = [R.blob(37, 53, k) for k in (0, 2, 11)]
    st = decode.stage_coefs(blobs, workers=1)
    assert st.status == [0, 0, 0]
    stride = st.slots.shape[1]
    coefs = torch.from_numpy(st.slots).cuda()
    good = backend.jpeg_reconstruct(coefs, st.descs, 37, 53).cpu().numpy()
    assert np.array_equal(good, decode.decode_batch(blobs))

    def refused(edit):
        descs = (_lib.LlfeJpegDesc * 3).from_buffer_copy(st.descs)
        edit(descs)
        out = torch.full((3, 37, 53, 3), 77, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(_lib.LlfeError) as e:
            backend.jpeg_reconstruct(coefs, descs, 37, 53, out=out)
        assert e.value.code == _lib.LLFE_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((out == 77).all())  # no kernel ran: not even the valid images were written

    def past_slot(d):
        d[1].comp[2].coef_offset = stride - 64

    def negative(d):
        d[0].comp[0].coef_offset = -128

    def quant_past_slot(d):
        d[2].comp[0].quant_offset = stride

    def grid_too_small(d):
        d[0].comp[0].blocks_w -= 1

    def unknown_class(d):
        d[1].sampling = 9

    def huge_grid(d):
        d[0].comp[1].blocks_h = 8000

    def wrong_chroma_size(d):
        d[0].comp[1].width += 1

    for edit in (past_slot, negative, quant_past_slot, grid_too_small, unknown_class, huge_grid, wrong_chroma_size):
        refused(edit)
