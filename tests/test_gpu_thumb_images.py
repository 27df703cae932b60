"""llfe_thumbnail_pil_images on the device (thumb_images.hip): every result byte-identical to
Pillow's own Image.thumbnail, for the case tables of tests/thumb_images_cases.py (whose branches
tests/test_thumb_images_inputs.py proves on the CPU), for every kind of source, for a shared
plan, across staging chunks, at large sizes and through ImageProcessor.auto_process_images."""
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import backend as B
from tests import resize_cases as RC
from tests import thumb_images_cases as TC

pytestmark = pytest.mark.gpu


def _same(got, exp, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    exp = np.asarray(exp)
    assert got.shape == exp.shape, f"{what}: shape {got.shape}, expected {exp.shape}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        where = [(tuple(int(v) for v in p), int(got[tuple(p)]), int(exp[tuple(p)])) for p in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {exp.size} bytes differ; (index, got, expected): {where}")


def _check(got, name):
    cases, exp = TC.TABLES[name][1], TC.expected(name)
    assert len(got) == len(exp)
    for c, g, e in zip(cases, got, exp):
        assert g.is_cuda and g.data_ptr() % 16 == 0
        _same(g, e, f"{name} {c.id}")


@pytest.mark.parametrize("name", list(TC.TABLES))
def test_parity_with_pillow_from_numpy(backend, name):
    box = TC.TABLES[name][0]
    if name == "box300x200":
        # the 200 x 300 results stand on the tile seams: at least three tiles in each axis and
        # a partial last one
        tw, th, _, _ = B.thumbnail_images_tiling()
        assert sum((c.oh, c.ow) == (200, 300) for c in TC.TABLES[name][1]) >= 3
        assert 300 // tw >= 3 and 300 % tw != 0 and 200 // th >= 3 and 200 % th != 0
    _check(backend.thumbnail_pil_images([np.array(x) for x in TC.batch(name)], *box), name)


def _as_kind(torch, x, kind):
    """The image as one kind of source; the bytes are the same."""
    h, w = x.shape[:2]
    if kind == "packed":
        return torch.from_numpy(np.array(x)).cuda()
    if kind == "crop":  # rows strided: big[:, 5:5 + w]
        big = torch.full((h, w + 9, 3), 77, dtype=torch.uint8, device="cuda")
        big[:, 5:5 + w] = torch.from_numpy(np.array(x)).cuda()
        return big[:, 5:5 + w]
    if kind == "offset3":  # starts 3 bytes into its allocation
        flat = torch.empty(h * w * 3 + 3, dtype=torch.uint8, device="cuda")
        flat[3:] = torch.from_numpy(np.array(x)).cuda().reshape(-1)
        t = flat[3:].view(h, w, 3)
        assert t.data_ptr() % 4 == 3
        return t
    return np.array(x)  # host


@pytest.mark.parametrize("name", list(TC.TABLES))
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_source_kinds(backend, name, shift):
    import torch

    kinds = ("packed", "crop", "offset3", "host")
    box = TC.TABLES[name][0]
    srcs = [_as_kind(torch, x, kinds[(k + shift) % 4]) for k, x in enumerate(TC.batch(name))]
    _check(backend.thumbnail_pil_images(srcs, *box), name)


def test_one_plan_three_images(backend):
    """One size three times, different contents, among other sizes: the shared plan must not
    mix the images."""
    h, w = 301, 212
    imgs = [RC.images(h, w, 3, seed=s)[0] for s in (5, 6, 7)]
    other = TC.image(50, 70, 0)
    batch = [imgs[0], other, imgs[1], imgs[2], other]
    got = backend.thumbnail_pil_images([np.array(x) for x in batch], *TC.BOX_SMALL)
    exp = [TC.pil_thumbnail(x, TC.BOX_SMALL) for x in batch]
    assert not np.array_equal(exp[0], exp[2]) and not np.array_equal(exp[2], exp[3])
    for i, (g, e) in enumerate(zip(got, exp)):
        _same(g, e, f"image {i}")


def test_staging_chunks(backend, monkeypatch):
    """Host sources under a staging budget that forces several chunks: a chunk's images overwrite
    the workspace of the one before."""
    name = "box50"
    box = TC.TABLES[name][0]
    srcs = [np.array(x) for x in TC.batch(name)]
    monkeypatch.setenv("LLFE_THUMB_STAGE_BYTES", "70000")
    backend.set_profiling(True)
    try:
        got = backend.thumbnail_pil_images(srcs, *box)
        launches = backend.kernel_stats()["k_thumb_lanczos"]["launches"]
    finally:
        backend.set_profiling(False)
    assert launches >= 3, launches  # one resample launch per chunk
    _check(got, name)


def test_short_destination_is_left_untouched(backend):
    import torch

    box = TC.BOX_SMALL
    srcs = [np.array(x) for x in TC.batch("box50")]
    descs, keep, _, _, _ = B._image_descs(srcs, backend.device)
    lay, total = B.thumbnail_images_layout(srcs, *box)
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = (L.LlfeThumbOut * len(srcs))()
    with backend._lock:
        rc = backend._lib.llfe_thumbnail_pil_images(backend.ctx, descs.ctypes.data, len(srcs), box[0], box[1],
                                                    dst.data_ptr(), total - 1, outs, None)
    torch.cuda.synchronize()
    assert rc == L.LLFE_ERR_CAPACITY
    assert bool((dst == 0xA5).all())
    with backend._lock:
        rc = backend._lib.llfe_thumbnail_pil_images(backend.ctx, descs.ctypes.data, len(srcs), box[0], box[1],
                                                    dst.data_ptr(), total, outs, None)
    assert rc == L.LLFE_OK
    assert [(o.offset, o.height, o.width, o.resized) for o in outs] == lay
    for c, o, e in zip(TC.CASES_SMALL, outs, TC.expected("box50")):
        _same(dst[o.offset:o.offset + e.size].view(*e.shape), e, c.id)
    # n == 0 is fine and writes nothing
    with backend._lock:
        assert backend._lib.llfe_thumbnail_pil_images(backend.ctx, None, 0, 50, 50, None, 0, None, None) == L.LLFE_OK
    assert backend.thumbnail_pil_images([]) == []


def test_large_sizes(backend):
    """2160 x 3840, 3024 x 4032 and 5000 x 2400 at the default box in one call."""
    import torch

    src, exp = TC.large_batch()
    got = backend.thumbnail_pil_images([torch.from_numpy(np.array(x)).cuda() for x in src], *TC.DEFAULT_BOX)
    for (h, w), g, e in zip(TC.LARGE_SIZES, got, exp):
        _same(g, e, f"{h}x{w}")


def test_auto_process_images_on_the_device(backend):
    from low_level_feature_extraction_amd.image_processor import ImageProcessor
    from low_level_feature_extraction_amd.pipeline import run_batch
    from low_level_feature_extraction_amd.synth import encode_png

    sizes = ((431, 647), (50, 70), (883, 1321))
    blobs = [encode_png(np.array(TC.image(h, w, k))) for k, (h, w) in enumerate(sizes)]
    blobs.insert(1, b"junk, not an image")
    host = ImageProcessor.auto_process_images(blobs, 300, 200)
    dev = ImageProcessor.auto_process_images(blobs, 300, 200, device=True)
    assert len(dev) == len(host) == 4
    assert isinstance(host[1], ValueError) and isinstance(dev[1], ValueError) and str(dev[1]) == str(host[1])
    good = [0, 2, 3]
    for i in good:
        assert dev[i].is_cuda
        _same(dev[i], host[i], f"image {i}")
    feats = ("shapes", "shadows")
    a = run_batch([dev[i] for i in good], feats, seed=0, index_base=0)
    b = run_batch([host[i] for i in good], feats, seed=0, index_base=0)
    assert a == b
