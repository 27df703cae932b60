"""EXIF orientation applied by the device reconstruction of a mixed-size batch
(csrc/jpeg_images.hip behind decode.decode_images_device(orient="device")): every image the same
bytes as decode.decode_bgr, which transposes on the host, for every sampling class and every
orientation on the kernel's tile seams, with the device entropy decode, with restart markers,
among neighbours the route hands back, through chunked staging, into a tensor with guard bytes
between the results, and downstream through auto_process_images.  An orientation outside 1 .. 8
and an output that is too small are refused by the host check before any launch."""
import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib, decode, synth
from low_level_feature_extraction_amd.backend import jpeg_images_tiling
from tests import jpeg_orient_cases as OC
from tests import jpeg_restate as R

pytestmark = pytest.mark.gpu

CLASSES = {R.S444: dict(subsampling=0), R.S422: dict(subsampling=1), R.S420: dict(subsampling=2), R.GRAY: dict(gray=True)}


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


def _blob(arr, o, gray=False, **kw):
    return OC.jpeg(arr[:, :, 1].copy() if gray else arr, o, **kw)


def _seam_sizes(cls):
    tw, th = jpeg_images_tiling(cls)
    return [(1, 1), (th, tw), (th + 1, tw + 1), (th - 1, tw + 2), (2 * th + 3, 2 * tw - 1), (5, 3 * tw + 6),
            (3 * th + 6, 5)]


_CACHE = {}


def _seam_blobs(restart=False):
    """Every seam size x every orientation of every class, in a fixed shuffled order: 224 images
    from 1 x 1 to 131 x 255."""
    if restart not in _CACHE:
        blobs = []
        for cls in (R.S444, R.S422, R.S420, R.GRAY):
            kw = dict(CLASSES[cls], quality=75)
            if restart:
                kw["restart_marker_blocks"] = 3
            for h, w in _seam_sizes(cls):
                arr = OC.pixels(h, w, 1000 * cls + 7 * h + w) if min(h, w) < 32 else \
                    synth.synth_numpy(cls, h, w, seed=4)[:, :, ::-1].copy()
                blobs += [_blob(arr, o, **kw) for o in OC.ORIENTATIONS]
        order = np.random.default_rng(224).permutation(len(blobs))
        _CACHE[restart] = [blobs[i] for i in order]
    return _CACHE[restart]


def test_tile_seams_every_orientation(backend):
    """Result rows that are and are not 4-byte aligned in both shapes, a last tile one pixel wide
    or high, one-pixel results; one call, nothing through the fallback."""
    blobs = _seam_blobs()
    st = decode.stage_coefs_images(blobs, workers=2, orient=True)
    assert st.layout_status == [0] * len(blobs) and st.status == [0] * len(blobs)
    assert sorted({(d.sampling, o) for d, o in zip(st.descs, st.orientation)}) == \
        [(c, o) for c in (R.GRAY, R.S444, R.S422, R.S420) for o in OC.ORIENTATIONS]
    _same(blobs, orient="device")


def test_tile_seams_device_entropy(backend):
    blobs = _seam_blobs()
    sb = decode.stage_bytes_images(blobs, workers=2, orient=True)
    assert sb.layout_status == [0] * len(blobs) and sb.status == [0] * len(blobs)
    _same(blobs, orient="device", entropy="device")


def test_tile_seams_device_entropy_restarts(backend):
    blobs = _seam_blobs(restart=True)
    sb = decode.stage_bytes_images(blobs, workers=2, restarts=True, orient=True)
    assert sb.layout_status == [0] * len(blobs) and sb.status == [0] * len(blobs)
    assert sum(s.restart_interval != 0 for s in sb.scans) > len(blobs) // 2
    _same(blobs, orient="device", entropy="device", restarts=True)


def test_batch_with_neighbours(backend):
    """Oriented and upright files, a PNG, a CMYK file, junk, and a progressive oriented file that
    the device entropy decode hands to the host coefficient path and the device still orients."""
    sizes = [(70, 130), (33, 200), (64, 64), (40, 56), (130, 136), (37, 53), (48, 80)]
    imgs = [synth.synth_numpy(i, h, w, seed=9) for i, (h, w) in enumerate(sizes)]
    rgb = [im[:, :, ::-1].copy() for im in imgs]
    cmyk = OC.jpeg(np.random.default_rng(3).integers(0, 256, (20, 30, 4), dtype=np.uint8), 6)
    blobs = [OC.jpeg(rgb[0], 6, quality=90, subsampling=2), OC.jpeg(rgb[1], None, quality=80, subsampling=1),
             synth.encode_png(imgs[3]), OC.jpeg(rgb[2], 3, quality=70, subsampling=0), cmyk,
             OC.jpeg(rgb[4], 8, quality=85, subsampling=2, progressive=True), b"\xff\xd8\xffjunk",
             OC.jpeg(rgb[5][:, :, 1].copy(), 5, quality=85), OC.jpeg(rgb[6], 7, quality=60, subsampling=1)]
    sb = decode.stage_bytes_images(blobs, workers=2, orient=True)
    assert [rc == 0 for rc in sb.status] == [True, True, False, True, False, False, False, True, True]
    st = decode.stage_coefs_images(blobs, workers=2, orient=True)
    assert [rc == 0 for rc in st.status] == [True, True, False, True, False, True, False, True, True]
    assert st.orientation == [6, 1, 1, 3, 1, 8, 1, 5, 7]
    for kw in (dict(entropy="device"), dict()):
        got = decode.decode_images_device(blobs, workers=2, orient="device", **kw)
        assert isinstance(got[6], decode.DecodeError)
        for i, b in enumerate(blobs):
            if i != 6:
                want = decode.decode_bgr(b)
                assert tuple(got[i].shape) == want.shape and np.array_equal(got[i].cpu().numpy(), want), (i, kw)
        assert tuple(got[0].shape) == (130, 70, 3) and tuple(got[5].shape) == (136, 130, 3)  # transposed
        assert tuple(got[3].shape) == (64, 64, 3) and tuple(got[8].shape) == (80, 48, 3)


def test_chunked_staging(backend, monkeypatch):
    """Five oriented 40 x 56 images, the bound at two of the smallest slots: at least three
    chunks, oriented images in every one."""
    arr = [OC.pixels(40, 56, 60 + i) for i in range(5)]
    blobs = [OC.jpeg(a, (6, 8, 3, 5, 2)[i], quality=50 + 10 * i, subsampling=i % 3) for i, a in enumerate(arr)]
    slot = [m.slot_bytes for m in decode.images_layout(blobs, orient=True)[0]]
    assert min(slot) > 0 and max(slot) > min(slot) and sum(slot) > 4 * min(slot)
    one = _same(blobs, orient="device")
    monkeypatch.setenv("LLFE_JPEG_STAGE_BYTES", str(2 * min(slot)))
    got = _same(blobs, orient="device")
    _same(blobs, orient="device", entropy="device")
    assert all(a.data_ptr() - got[0].data_ptr() == b.data_ptr() - one[0].data_ptr() for a, b in zip(got, one))


def _staged_on_device(blobs):
    import torch

    st = decode.stage_coefs_images(blobs, workers=1, orient=True)
    assert st.status == [0] * len(blobs)
    return st, torch.from_numpy(st.slots[:st.used_bytes].copy()).cuda()


def test_guard_bytes_between_the_results(backend):
    """The results 16 bytes apart in a tensor of 77s: a store past a row's or a result's end, in
    either shape, lands in a gap."""
    import torch

    blobs = []
    for cls in (R.S420, R.S444, R.GRAY, R.S422):
        tw, th = jpeg_images_tiling(cls)
        for k, (h, w) in enumerate(((th + 1, tw + 3), (7, tw + 2), (th + 6, 5), (th, tw))):
            blobs += [_blob(OC.pixels(h, w, 11 * h + w), o, quality=70, **CLASSES[cls])
                      for o in ((2, 5, 7), (3, 6, 8), (4, 6, 7), (1, 8, 3))[k]]
    st, coefs = _staged_on_device(blobs)
    off = 16
    for m in st.images:
        m.out_offset = off
        off = ((off + m.height * m.width * 3 + 15) & ~15) + 16
    out = torch.full((off,), 77, dtype=torch.uint8, device="cuda:0")
    got = backend.jpeg_reconstruct_images(coefs, st.images, st.descs, out, st.orientation).cpu().numpy()
    used = np.zeros(off, bool)
    for m, b in zip(st.images, blobs):
        want = decode.decode_bgr(b)
        assert want.size == m.height * m.width * 3
        assert np.array_equal(got[m.out_offset: m.out_offset + want.size].reshape(want.shape), want)
        used[m.out_offset: m.out_offset + want.size] = True
    assert bool((got[~used] == 77).all()) and int((~used).sum()) >= 16 * (len(blobs) + 1)


def test_refused_before_any_launch(backend):
    import torch

    blobs = [_blob(OC.pixels(37, 53, 1), 6, subsampling=2), _blob(OC.pixels(17, 33, 2), 3, subsampling=0),
             _blob(OC.pixels(16, 16, 3), None, gray=True)]
    st, coefs = _staged_on_device(blobs)
    off = 0
    for m in st.images:
        m.out_offset = off
        off = (off + m.height * m.width * 3 + 15) & ~15

    def refused(orientation, code, capacity=off):
        out = torch.full((capacity,), 77, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(_lib.LlfeError) as e:
            backend.jpeg_reconstruct_images(coefs, st.images, st.descs, out, orientation)
        assert e.value.code == code, orientation
        torch.cuda.synchronize()
        assert bool((out == 77).all()), orientation  # no kernel ran: not even the valid images were written

    refused([6, 9, 1], _lib.LLFE_ERR_INVALID)
    refused([0, 3, 1], _lib.LLFE_ERR_INVALID)
    refused([6, 3, 255], _lib.LLFE_ERR_INVALID)
    # a result laid out for either shape needs its h * w * 3 bytes
    refused(st.orientation, _lib.LLFE_ERR_CAPACITY, st.images[2].out_offset + 16 * 16 * 3 - 1)
    refused([1, 1, 1], _lib.LLFE_ERR_CAPACITY, st.images[2].out_offset + 16 * 16 * 3 - 1)
    # the thin call's own argument check
    out = torch.zeros(off, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError):
        backend.jpeg_reconstruct_images(coefs, st.images, st.descs, out, [6, 3])
    good = backend.jpeg_reconstruct_images(coefs, st.images, st.descs, out, st.orientation).cpu().numpy()
    for m, b in zip(st.images, blobs):
        want = decode.decode_bgr(b)
        assert np.array_equal(good[m.out_offset: m.out_offset + want.size].reshape(want.shape), want)


def test_downstream_equality(backend):
    from low_level_feature_extraction_amd.image_processor import ImageProcessor

    sizes = [(128, 160), (96, 200), (130, 136), (64, 64)]
    imgs = [synth.synth_numpy(i, h, w, seed=21) for i, (h, w) in enumerate(sizes)]
    blobs = [OC.jpeg(im[:, :, ::-1].copy(), (6, 3, None, 6)[i], quality=85, subsampling=(2, 1, 0, 2)[i])
             for i, im in enumerate(imgs)]
    for kw in (dict(), dict(entropy="device")):
        dev = ImageProcessor.auto_process_images(blobs + [b"junk"], 50, 40, device=True, decode="device", orient="device",
                                                 **kw)
        host = ImageProcessor.auto_process_images(blobs + [b"junk"], 50, 40, device=True, decode="host")
        assert len(dev) == len(host) == 5
        for x, y in zip(dev[:4], host[:4]):
            assert x.is_cuda and tuple(x.shape) == tuple(y.shape) and np.array_equal(x.cpu().numpy(), y.cpu().numpy())
        assert isinstance(dev[4], ValueError) and isinstance(host[4], ValueError) and str(dev[4]) == str(host[4])


def test_defaults_hand_an_oriented_file_back(backend):
    arr = synth.synth_numpy(2, 48, 80, seed=9)[:, :, ::-1].copy()
    blobs = [OC.jpeg(arr, 6, quality=85, subsampling=2), OC.jpeg(arr, None, quality=85, subsampling=2)]
    for st in (decode.stage_coefs_images(blobs, workers=1), decode.stage_bytes_images(blobs, workers=1)):
        assert st.status[0] != 0 and st.layout_status[0] != 0 and st.status[1] == 0 and st.orientation == [1, 1]
    got = _same(blobs)
    assert tuple(got[0].shape) == (80, 48, 3)
    dev = _same(blobs, orient="device")
    assert np.array_equal(got[0].cpu().numpy(), dev[0].cpu().numpy())
