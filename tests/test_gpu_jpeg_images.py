"""JPEG decode of a mixed-size batch on the device (csrc/jpeg_images.hip behind
decode.decode_images_device): every image the same bytes as the host decoder
(decode.decode_bgr, which tests/test_jpeg_coefs.py pins against the installed libjpeg-turbo),
for every case of tests/jpeg_restate.py in one launch, on the kernel's tile seams for each
sampling class, for narrow chroma, hand-made tables, a batch with host fallbacks of other
sizes, chunked staging, and downstream through process_images and auto_process_images.  A
record that points outside its slot, the coefficient buffer or the output is refused by the
host check before any launch."""
import dataclasses
import io

import numpy as np
import pytest
from PIL import Image

from low_level_feature_extraction_amd import _lib, decode, synth
from low_level_feature_extraction_amd.backend import jpeg_images_tiling
from tests import jpeg_restate as R

pytestmark = pytest.mark.gpu


def _same(blobs, **kw):
    """decode_images_device against decode_bgr per image; -> the list of device tensors."""
    got = decode.decode_images_device(blobs, workers=2, **kw)
    assert len(got) == len(blobs)
    base = None
    for i, b in enumerate(blobs):
        want = decode.decode_bgr(b)
        t = got[i]
        assert t.is_cuda and tuple(t.shape) == want.shape, (i, tuple(t.shape), want.shape)
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        base = t.untyped_storage().data_ptr() if base is None else base
        assert t.untyped_storage().data_ptr() == base  # views into one packed tensor
        g = t.cpu().numpy()
        assert np.array_equal(g, want), f"image {i} ({want.shape}) differs at {np.argwhere(g != want)[:4].tolist()}"
    return got


def test_case_list_ragged(backend):
    """All of SIZES x SETTINGS in a fixed shuffled order, 98 images from 1 x 1 to 240 x 321 with
    every sampling class, in one launch."""
    order = np.random.default_rng(98).permutation(len(R.CASES))
    blobs = [R.blob(*R.CASES[i]) for i in order]
    st = decode.stage_coefs_images(blobs, workers=2)
    # all reconstructed on the device, none by the fallback
    assert st.layout_status == [0] * len(blobs) and st.status == [0] * len(blobs)
    _same(blobs)


@pytest.mark.parametrize("sub", [0, 1, 2, "gray"])
def test_tile_seams(backend, sub):
    """Sizes on the tile of the class: a right / lower halo clamped inside the tile, a halo that
    is a real sample in a block of the next tile, a chroma grid of 8k + 1 samples, rows that are
    and are not 4-byte aligned, a last tile one pixel wide or high."""
    cls = {0: R.S444, 1: R.S422, 2: R.S420, "gray": R.GRAY}[sub]
    tw, th = jpeg_images_tiling(cls)
    blobs = []
    for h, w in ((th, tw), (th + 1, tw + 1), (th - 1, tw + 2), (2 * th + 3, 2 * tw - 1), (5, 3 * tw + 6)):
        rng = np.random.default_rng(h * w)
        a = synth.synth_numpy(0, h, w, seed=2)[:, :, ::-1].copy()
        b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if sub == "gray":
            blobs += [R.jpeg(a[:, :, 1].copy(), quality=85), R.jpeg(b[:, :, 1].copy(), quality=40)]
        else:
            blobs += [R.jpeg(a, quality=85, subsampling=sub), R.jpeg(b, quality=40, subsampling=sub)]
    st = decode.stage_coefs_images(blobs, workers=2)
    assert st.status == [0] * len(blobs) and all(d.sampling == cls for d in st.descs)
    _same(blobs)


def test_narrow_chroma(backend):
    """Widths 1..6 x heights 1, 2, 5, 17 at 4:2:0 and 4:2:2: a chroma width <= 2 (plain
    replication) and 3 (the first width with the triangle filter)."""
    rng = np.random.default_rng(6)
    blobs = [R.jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), quality=90, subsampling=sub)
             for sub in (2, 1) for w in range(1, 7) for h in (1, 2, 5, 17)]
    assert decode.stage_coefs_images(blobs, workers=2).status == [0] * len(blobs)
    _same(blobs)


def test_hand_made_tables(backend):
    """Quantisation tables scaled by 5 (saturation), 40 and 255 (16-bit products and sums wrap,
    the whole-block DC shortcut differs from the full pass), mixed with 17 x 33 images."""
    blobs = []
    for k in (2, 6, 13, 3):
        for f in (5, 40, 255):
            blobs += [R.scaled_tables(R.blob(37, 53, k), f), R.blob(17, 33, k)]
    assert decode.stage_coefs_images(blobs, workers=2).status == [0] * len(blobs)
    _same(blobs)


def test_mixed_batch_with_fallbacks(backend):
    """The twelve blobs of test_gpu_jpeg_recon's mixed batch, each with its own size from
    9 x 260 down to 72 x 100; the EXIF image is a non-square orientation 6, so its result has the
    transposed size; one blob is garbage."""
    sizes = [(9, 260), (70, 130), (33, 200), (64, 64), (12, 256), (40, 56), (130, 136), (5, 300), (24, 24), (37, 53),
             (48, 80), (72, 100)]
    imgs = [synth.synth_numpy(i, h, w, seed=9) for i, (h, w) in enumerate(sizes)]
    rgb = [im[:, :, ::-1].copy() for im in imgs]
    ex = Image.Exif()
    ex[0x0112] = 6
    rot = io.BytesIO()
    Image.fromarray(rgb[10]).save(rot, "JPEG", exif=ex.tobytes())
    blobs = [R.jpeg(rgb[0], quality=90, subsampling=0), R.jpeg(rgb[1], quality=80, subsampling=1),
             R.jpeg(rgb[2], quality=70, subsampling=2), R.jpeg(rgb[3][:, :, 1].copy(), quality=85),
             R.jpeg(rgb[4], quality=88, progressive=True), synth.encode_png(imgs[5]),
             R.jpeg(rgb[6], quality=30, subsampling=2, optimize=True), R.jpeg(rgb[7], quality=95, subsampling=1),
             R.jpeg(rgb[8], quality=75, restart_marker_blocks=2), synth.encode_png(imgs[9]), rot.getvalue(),
             R.jpeg(rgb[11], quality=1, subsampling=0)]
    st = decode.stage_coefs_images(blobs, workers=3)
    assert [rc != 0 for rc in st.status] == [i in (5, 9, 10) for i in range(12)]
    got = _same(blobs)
    assert np.array_equal(got[5].cpu().numpy(), imgs[5]) and np.array_equal(got[9].cpu().numpy(), imgs[9])
    assert tuple(got[10].shape) == (80, 48, 3)  # transposed
    # a blob nothing decodes: a DecodeError in its place, every other place as before
    with_junk = blobs[:4] + [b"\xff\xd8\xffjunk"] + blobs[4:]
    res = decode.decode_images_device(with_junk, workers=2)
    assert isinstance(res[4], decode.DecodeError)
    for i, b in enumerate(with_junk):
        if i != 4:
            assert np.array_equal(res[i].cpu().numpy(), decode.decode_bgr(b)), i


def test_chunked_staging(backend, monkeypatch):
    """The staging buffer is bounded and a batch above the bound goes through it in chunks of
    whole images: five 40 x 56 images, the bound at two of the smallest slots, are at least three
    chunks; an image that alone exceeds the bound takes the host decoder."""
    rng = np.random.default_rng(11)
    blobs = [R.jpeg(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), quality=50 + 10 * i, subsampling=i % 3)
             for i in range(5)]
    slot = [m.slot_bytes for m in decode.images_layout(blobs)[0]]
    monkeypatch.setenv("LLFE_JPEG_STAGE_BYTES", str(2 * min(slot)))
    assert max(slot) > min(slot) and sum(slot) > 4 * min(slot)  # (4:4:4 slots are larger: >= 3 chunks)
    got = _same(blobs)
    monkeypatch.setenv("LLFE_JPEG_STAGE_BYTES", str(max(slot) - 16))  # the 4:4:4 images alone exceed it
    _same(blobs)
    monkeypatch.delenv("LLFE_JPEG_STAGE_BYTES")
    one = _same(blobs)
    assert all(a.data_ptr() - got[0].data_ptr() == b.data_ptr() - one[0].data_ptr() for a, b in zip(got, one))


def test_refused_before_any_launch(backend):
    import torch

    blobs = [R.blob(37, 53, 0), R.blob(17, 33, 2), R.blob(16, 16, 11)]
    st = decode.stage_coefs_images(blobs, workers=1)
    assert st.status == [0, 0, 0]
    off = 0
    for m in st.images:
        m.out_offset = off
        off = (off + m.height * m.width * 3 + 15) & ~15
    coefs = torch.from_numpy(st.slots[:st.used_bytes].copy()).cuda()
    good = backend.jpeg_reconstruct_images(coefs, st.images, st.descs, torch.zeros(off, dtype=torch.uint8, device="cuda:0"))
    good = good.cpu().numpy()
    for m, b in zip(st.images, blobs):
        got = good[m.out_offset: m.out_offset + m.height * m.width * 3].reshape(m.height, m.width, 3)
        assert np.array_equal(got, decode.decode_bgr(b))

    def refused(edit, code=_lib.LLFE_ERR_INVALID, capacity=off):
        images = (_lib.LlfeJpegImage * 3).from_buffer_copy(st.images)
        descs = (_lib.LlfeJpegDesc * 3).from_buffer_copy(st.descs)
        edit(images, descs)
        out = torch.full((capacity,), 77, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(_lib.LlfeError) as e:
            backend.jpeg_reconstruct_images(coefs, images, descs, out)
        assert e.value.code == code, edit.__name__
        torch.cuda.synchronize()
        assert bool((out == 77).all()), edit.__name__  # no kernel ran: not even the valid images were written

    def past_slot(m, d):
        d[1].comp[2].coef_offset = m[1].slot_bytes - 64

    def negative(m, d):
        d[0].comp[0].coef_offset = -128

    def quant_at_slot_end(m, d):
        d[2].comp[0].quant_offset = m[2].slot_bytes

    def grid_too_small(m, d):
        d[0].comp[0].blocks_w -= 1

    def unknown_class(m, d):
        d[1].sampling = 9

    def huge_grid(m, d):
        d[0].comp[1].blocks_h = 8000

    def wrong_chroma_size(m, d):
        d[0].comp[1].width += 1

    def taller_record(m, d):
        m[1].height += 1

    def slot_past_coefs(m, d):
        m[2].slot_offset = st.used_bytes

    def odd_out_offset(m, d):
        m[1].out_offset += 1

    def overlapping_results(m, d):
        m[2].out_offset = m[1].out_offset + 16

    for edit in (past_slot, negative, quant_at_slot_end, grid_too_small, unknown_class, huge_grid, wrong_chroma_size,
                 taller_record, slot_past_coefs, odd_out_offset, overlapping_results):
        refused(edit)
    refused(lambda m, d: None, _lib.LLFE_ERR_CAPACITY, st.images[2].out_offset + 16 * 16 * 3 - 1)
    # the thin call's own argument checks
    out = torch.zeros(off, dtype=torch.uint8, device="cuda:0")
    for bad in (lambda: backend.jpeg_reconstruct_images(coefs.cpu(), st.images, st.descs, out),
                lambda: backend.jpeg_reconstruct_images(coefs, st.images, st.descs, out.cpu()),
                lambda: backend.jpeg_reconstruct_images(coefs, st.images, st.descs[:2], out),
                lambda: backend.jpeg_reconstruct_images(coefs.view(-1, 16), st.images, st.descs, out)):
        with pytest.raises(ValueError):
            bad()


def test_downstream_equality(backend):
    from low_level_feature_extraction_amd.image_processor import ImageProcessor

    sizes = [(128, 160), (96, 200), (130, 136), (64, 64)]
    imgs = [synth.synth_numpy(i, h, w, seed=21) for i, (h, w) in enumerate(sizes)]
    blobs = [R.jpeg(im[:, :, ::-1].copy(), quality=85, subsampling=(2, 1, 0, 2)[i]) for i, im in enumerate(imgs)]
    feats = ("colors", "shapes", "shadows")
    a = backend.process_images(decode.decode_images_device(blobs), feats, seed=5)
    b = backend.process_images([decode.decode_bgr(x) for x in blobs], feats, seed=5)
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        for f in dataclasses.fields(x):
            u, v = getattr(x, f.name), getattr(y, f.name)
            assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v, f.name
    dev = ImageProcessor.auto_process_images(blobs + [b"junk"], 50, 40, device=True, decode="device")
    host = ImageProcessor.auto_process_images(blobs + [b"junk"], 50, 40, device=True, decode="host")
    assert len(dev) == len(host) == 5
    for x, y in zip(dev[:4], host[:4]):
        assert x.is_cuda and tuple(x.shape) == tuple(y.shape) and np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert isinstance(dev[4], ValueError) and isinstance(host[4], ValueError) and str(dev[4]) == str(host[4])
