"""llfe_preprocess_images / llfe_resize_cv_images on the device (cvresize_images.hip): every
result byte-identical to the oracle's cv_resize and to Backend.resize_cv, the per-image route, for
the case tables of tests/preprocess_images_cases.py (whose plans
tests/test_preprocess_images_inputs.py proves on the CPU), on the tile seams, for every kind of
source, for a shared plan, across staging chunks, at large sizes and through the Python surface."""
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import backend as B
from tests import preprocess_images_cases as PC
from tests import resize_cases as RC

pytestmark = pytest.mark.gpu


def _same(got, exp, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    exp = exp.cpu().numpy() if hasattr(exp, "cpu") else np.asarray(exp)
    assert got.shape == exp.shape, f"{what}: shape {got.shape}, expected {exp.shape}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        where = [(tuple(int(v) for v in p), int(got[tuple(p)]), int(exp[tuple(p)])) for p in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {exp.size} bytes differ; (index, got, expected): {where}")


def _check(got, exp, ids):
    assert len(got) == len(exp)
    for g, e, i in zip(got, exp, ids):
        assert g.is_cuda and g.data_ptr() % 16 == 0, i
        _same(g, e, i)


# ------------------------------------------------------------------ 1. the stage entry, smallest shapes
def _stage_items(interps):
    """(id, image, (ow, oh, interp), expected) of every case of the interpolations, three images each."""
    items = []
    for c in PC.stage_cases():
        if c.interp in interps:
            for kind, x, e in zip(RC.IMAGE_KINDS, RC.cv_images(c), RC.cv_expected(c)):
                items.append((f"{c.id} {kind}", x, (c.ow, c.oh, c.interp), e))
    return items


@pytest.mark.parametrize("interps", [("area",), ("linear",), ("lanczos4",), ("area", "linear", "lanczos4")],
                         ids=lambda v: "+".join(v))
def test_stage_entry_on_the_smallest_shapes(backend, interps):
    items = _stage_items(interps)
    assert len(items) >= 9
    if len(interps) == 3:  # every kind in one call, interleaved: the launches per kind must not mix records
        items = [items[i] for i in np.random.default_rng(3).permutation(len(items))]
    got = backend.resize_cv_images([np.array(it[1]) for it in items], [it[2] for it in items])
    _check(got, [it[3] for it in items], [it[0] for it in items])


def test_stage_entry_refuses_cubic_and_bad_codes(backend):
    x = np.array(PC.image(7, 11))
    with pytest.raises(L.LlfeError) as e:
        backend.resize_cv_images([x, x], [(4, 3, "area"), (4, 3, "cubic")])
    assert e.value.code == L.LLFE_ERR_UNSUPPORTED and "image 1" in str(e.value)
    for bad in ((4, 3, 7), (0, 3, "area"), (4, -1, "linear")):
        with pytest.raises(L.LlfeError) as e:
            backend.resize_cv_images([x], [bad])
        assert e.value.code == L.LLFE_ERR_INVALID


# ------------------------------------------------------------------ 2. the rule's cases
@pytest.mark.parametrize("mode", PC.MODES)
def test_rule_cases_equal_the_oracle_and_the_per_image_route(backend, mode):
    cases = PC.rule_cases(mode)
    imgs, exp = PC.rule_batch(mode)
    got = backend.preprocess_images([np.array(x) for x in imgs], mode)
    _check(got, exp, [c.id for c in cases])
    for c, x, g in zip(cases, imgs, got):
        if c.resized:
            _same(g, backend.resize_cv(np.array(x), c.ow, c.oh, c.interp), f"{c.id} against resize_cv")


def test_zero_side_is_refused_and_names_the_image(backend):
    mode, h, w = PC.ZERO_SIDE
    with pytest.raises(L.LlfeError) as e:
        backend.preprocess_images([np.array(PC.image(6, 4000)), np.zeros((h, w, 3), np.uint8)], mode)
    assert e.value.code == L.LLFE_ERR_INVALID
    descs, keep, _, _, _ = B._image_descs([np.array(PC.image(6, 4000)), np.zeros((h, w, 3), np.uint8)], backend.device)
    import torch

    dst = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = (L.LlfeResizeOut * 2)()
    with backend._lock:
        rc = backend._lib.llfe_preprocess_images(backend.ctx, descs.ctypes.data, 2, 1, dst.data_ptr(), dst.numel(), outs, None)
        msg = backend._lib.llfe_last_error(backend.ctx)
    assert rc == L.LLFE_ERR_INVALID and b"image 1" in msg
    assert bool((dst == 0xA5).all())
    with pytest.raises(ValueError):
        backend.preprocess_images([np.array(PC.image(6, 4000))], "sharpest")


# ------------------------------------------------------------------ 3. tile seams
def test_tile_seams_small_tiles_and_the_global_arm(backend):
    tw, th, lds_rows = B.resize_cv_images_tiling()
    cases, imgs, exp = PC.seam_batch(tw, th)
    for c in cases[:PC.N_SEAM]:
        assert c.ow // tw >= 3 and c.ow % tw != 0 and c.oh // th >= 3 and c.oh % th != 0
    got = backend.resize_cv_images([np.array(x) for x in imgs], [(c.ow, c.oh, c.interp) for c in cases])
    _check(got, exp, [c.id for c in cases])


# ------------------------------------------------------------------ 4. source kinds
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
    if kind == "host_crop":  # host rows strided: the upload goes through a 2-D copy with this pitch
        big = np.full((h, w + 9, 3), 77, np.uint8)
        big[:, 5:5 + w] = x
        t = big[:, 5:5 + w]
        assert t.strides[0] == 3 * (w + 9)
        return t
    return np.array(x)  # host, packed


def _mixed_batch():
    """Every plan kind, a copy and odd row lengths: (images, sizes, expected, ids)."""
    tw, th, _ = B.resize_cv_images_tiling()
    cases, imgs, exp = PC.seam_batch(tw, th)
    pick = [0, 1, 2, 3, 4, 8, PC.N_SEAM + 1, PC.N_SEAM + 2]  # AREA x 2, AREA_FAST x 2, LINEAR, LANCZOS4, small tile, global arm
    imgs, exp, ids = [imgs[i] for i in pick], [exp[i] for i in pick], [cases[i].id for i in pick]
    sizes = [(cases[i].ow, cases[i].oh, cases[i].interp) for i in pick]
    same = PC.image(37, 53, 1)
    return imgs + [same], sizes + [(53, 37, "area")], exp + [same], ids + ["copy-37x53"]


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4])
def test_source_kinds(backend, shift):
    import torch

    kinds = ("packed", "crop", "offset3", "host", "host_crop")
    imgs, sizes, exp, ids = _mixed_batch()
    srcs = [_as_kind(torch, x, kinds[(k + shift) % 5]) for k, x in enumerate(imgs)]
    _check(backend.resize_cv_images(srcs, sizes), exp, ids)


# ------------------------------------------------------------------ 5. shared plans
def test_one_plan_three_images(backend):
    """One size three times, different contents, among other sizes: the shared plan must not mix
    the images."""
    h, w = 9, 4032
    imgs = [PC.image(h, w, k) for k in (0, 1, 2)]
    other = PC.image(6, 4000)
    batch = [imgs[0], other, imgs[1], imgs[2], other]
    got = backend.preprocess_images([np.array(x) for x in batch], "auto")
    exp = [PC.expected(h, w, 4, 2000, "area", 0), PC.expected(6, 4000, 3, 2000, "area", 0),
           PC.expected(h, w, 4, 2000, "area", 1), PC.expected(h, w, 4, 2000, "area", 2),
           PC.expected(6, 4000, 3, 2000, "area", 0)]
    assert not np.array_equal(exp[0], exp[2]) and not np.array_equal(exp[2], exp[3])
    _check(got, exp, [f"image {i}" for i in range(5)])


# ------------------------------------------------------------------ 6. staging chunks
def test_staging_chunks(backend, monkeypatch):
    """Host sources under a staging budget that forces several chunks: a chunk's images overwrite
    the workspace of the one before."""
    cases = [c for c in PC.rule_cases("auto") if c.kind == "AREA"]
    assert len(cases) >= 4
    imgs = [np.array(PC.image(c.h, c.w, k)) for k, c in enumerate(cases)]
    exp = [PC.expected(c.h, c.w, c.oh, c.ow, c.interp, k) for k, c in enumerate(cases)]
    monkeypatch.setenv("LLFE_RESIZE_STAGE_BYTES", "50000")  # every image a chunk of its own
    backend.set_profiling(True)
    try:
        got = backend.preprocess_images(imgs, "auto")
        launches = backend.kernel_stats()["k_cv_images_area"]["launches"]
    finally:
        backend.set_profiling(False)
    assert launches >= 3, launches  # one launch per chunk
    _check(got, exp, [c.id for c in cases])


# ------------------------------------------------------------------ 7. capacity and empty
def test_short_destination_is_left_untouched(backend):
    import torch

    mode = "auto"
    cases = [c for c in PC.rule_cases(mode) if c.h * c.w < 100000]
    srcs = [np.array(PC.image(c.h, c.w, k)) for k, c in enumerate(cases)]
    exp = [PC.expected(c.h, c.w, c.oh, c.ow, c.interp, k) for k, c in enumerate(cases)]
    descs, keep, _, _, _ = B._image_descs(srcs, backend.device)
    lay, total = B.preprocess_images_layout(srcs, mode)
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = (L.LlfeResizeOut * len(srcs))()
    with backend._lock:
        rc = backend._lib.llfe_preprocess_images(backend.ctx, descs.ctypes.data, len(srcs), 1, dst.data_ptr(),
                                                 total - 1, outs, None)
    torch.cuda.synchronize()
    assert rc == L.LLFE_ERR_CAPACITY
    assert bool((dst == 0xA5).all())
    with backend._lock:
        rc = backend._lib.llfe_preprocess_images(backend.ctx, descs.ctypes.data, len(srcs), 1, dst.data_ptr(),
                                                 total, outs, None)
    assert rc == L.LLFE_OK
    assert [(o.offset, o.height, o.width, o.interpolation, o.resized) for o in outs] == lay
    for c, o, e in zip(cases, outs, exp):
        _same(dst[o.offset:o.offset + e.size].view(*e.shape), e, c.id)
    # n == 0 is fine and writes nothing
    with backend._lock:
        assert backend._lib.llfe_preprocess_images(backend.ctx, None, 0, 1, None, 0, None, None) == L.LLFE_OK
        assert backend._lib.llfe_resize_cv_images(backend.ctx, None, 0, None, None, 0, None, None) == L.LLFE_OK
    assert backend.preprocess_images([]) == [] and backend.resize_cv_images([], []) == []


# ------------------------------------------------------------------ 8. large sizes
def test_large_sizes(backend):
    """3024 x 4032, 2160 x 3840 and 3000 x 4000 (AREA_FAST 2 x 2) under auto in one call."""
    import torch

    src, exp = PC.large_batch()
    got = backend.preprocess_images([torch.from_numpy(np.array(x)).cuda() for x in src], "auto")
    _check(got, exp, [f"{h}x{w}" for h, w in PC.LARGE_SIZES])


# ------------------------------------------------------------------ 9. the Python surface
def test_validate_and_preprocess_images(backend):
    from low_level_feature_extraction_amd.synth import encode_png
    from low_level_feature_extraction_amd.utils import preprocess_decoded, validate_and_preprocess_images
    import asyncio

    from low_level_feature_extraction_amd.utils import validate_and_preprocess_image

    sizes = ((9, 4032), (50, 70), (2001, 5))
    imgs = [np.array(PC.image(h, w, k)) for k, (h, w) in enumerate(sizes)]
    blobs = [encode_png(x) for x in imgs]
    blobs.insert(1, b"junk, not an image")
    host = validate_and_preprocess_images(blobs, "auto")
    dev = validate_and_preprocess_images(blobs, "auto", device=True)
    assert len(host) == len(dev) == 4
    with pytest.raises(Exception) as single:
        asyncio.run(validate_and_preprocess_image(blobs[1], "r", "auto"))
    for e in (host[1], dev[1]):
        assert type(e) is type(single.value) and str(e) == str(single.value)
    for i, x in zip((0, 2, 3), imgs):
        one = preprocess_decoded(x, "auto")
        assert isinstance(host[i], np.ndarray) and dev[i].is_cuda and dev[i].data_ptr() % 16 == 0
        _same(host[i], one, f"host {i}")
        _same(dev[i], one, f"device {i}")
    assert host[0].shape == (4, 2000, 3) and host[2].shape == (50, 70, 3) and host[3].shape == (2000, 4, 3)
    with pytest.raises(ValueError, match='decode="device" needs device=True'):
        validate_and_preprocess_images(blobs, "auto", decode="device")


@pytest.mark.parametrize("routes", ["one_pass", "grouped"])
def test_run_batch_one_pass_equals_per_image(backend, routes):
    from low_level_feature_extraction_amd.pipeline import run_batch

    feats = ("colors", "shapes", "shadows")
    imgs = [np.array(RC.images(40, 2600, 3)[0]), np.array(RC.images(30, 50, 3)[0]), np.array(RC.images(2600, 33, 3)[2])]
    kw = dict(preprocessing="auto", colors=routes, shapes=routes, seed=0, index_base=0, raw=True)
    a = run_batch(imgs, feats, preprocess="per_image", **kw)
    b = run_batch(imgs, feats, preprocess="one_pass", **kw)
    sizes = [(r.width, r.height) for r in a]
    assert sizes == [(r.width, r.height) for r in b]
    assert max(sizes[0]) == 2000 and sizes[1] == (50, 30) and max(sizes[2]) == 2000
    kw["raw"] = False
    assert run_batch(imgs, feats, preprocess="one_pass", **kw) == run_batch(imgs, feats, preprocess="per_image", **kw)
    for x, y in zip(a, b):
        for f in x.__dataclass_fields__:
            u, v = getattr(x, f), getattr(y, f)
            assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v, f
    with pytest.raises(ValueError):
        run_batch(imgs, feats, preprocess="twice")
