"""The shapes and shadows of a batch of images of any sizes in one device pass
(process_images(..., shapes="one_pass"), shape_masks_images, shadow_stats_images,
hysteresis_images): image i's mask and shadow sums equal the oracle's for its own size, and its
result equals a one-image call's and the size-grouped route's bit for bit, whatever shares the
pass with it."""
import ctypes as C
import functools

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import backend as B
from low_level_feature_extraction_amd import synth
from tests import hysteresis_cases as HC

pytestmark = pytest.mark.gpu

KERNELS = ("k_stencil", "k_hysteresis_dilate")
# the 240-column strip and its 8-column halo (240, 241, 256, 257, 479, 480, 481), the 216-row
# segment rule (216, 217, 433), the 64-pixel tile (64, 65, 63 x 65), the W & 3 vector path
# (widths 8, 12, 16, 200, 240, 256, 480 against the odd ones) and images smaller than the
# filters' reach (1 x 1 .. 11 x 12); widths from 488 on have `fast` waves, whose interior strip
# comes by direct-to-LDS loads: 3 x 488 (H < 6: REFLECT_101 bounces more than once), 13 x 728
# (strips 1 and 2) and 229 x 488 (two segments: the first one's last rows read the ring after
# the loads have stopped)
LADDER = [(1, 1), (2, 3), (5, 7), (11, 12), (64, 240), (65, 241), (40, 256), (40, 257), (216, 8), (217, 9), (433, 16),
          (30, 479), (30, 480), (30, 481), (63, 65), (130, 200), (3, 488), (13, 728), (229, 488)]
FEATS = [("shapes",), ("shadows",), ("shapes", "shadows")]


@functools.lru_cache(maxsize=None)
def _ladder():
    return tuple(synth.synth_numpy(i, h, w, seed=41) for i, (h, w) in enumerate(LADDER))


@functools.lru_cache(maxsize=None)
def _alternating():
    return tuple(synth.synth_numpy(i, (90, 150)[i % 2], (160, 96)[i % 2], seed=23) for i in range(7))


def _same(a, b, tag, colors=False):
    assert (a.width, a.height) == (b.width, b.height), tag
    assert (a.shadow_sum, a.shadow_count, a.shadow_level) == (b.shadow_sum, b.shadow_count, b.shadow_level), tag
    assert a.shapes == b.shapes and a.n_contours == b.n_contours, tag
    if colors:
        assert a.n_unique == b.n_unique and a.compactness == b.compactness and a.palette == b.palette, tag
        assert np.array_equal(a.centers_rgb, b.centers_rgb) and np.array_equal(a.counts, b.counts), tag


_ALONE = {}


def _alone(backend, name, imgs, feats, seed, base):
    """The one-image calls of a list, computed once per (list, features)."""
    key = (name, feats, seed, base)
    if key not in _ALONE:
        _ALONE[key] = [backend.process(im[None], feats, seed=seed, index_base=base + i)[0] for i, im in enumerate(imgs)]
    return _ALONE[key]


# ------------------------------------------------------------------ 1. masks against the oracle
@pytest.mark.parametrize("order", ["input", "reversed"])
def test_masks_and_shadow_sums_equal_the_oracle(backend, orc, order):
    imgs = list(_ladder())
    if order == "reversed":
        imgs = imgs[::-1]
    masks = backend.shape_masks_images(imgs)
    sums, cnts = backend.shadow_stats_images(imgs)
    assert len(masks) == len(imgs)
    for i, im in enumerate(imgs):
        assert masks[i].shape == im.shape[:2]
        assert np.array_equal(masks[i], orc.shape_mask(im)), (order, i, im.shape)
        assert (int(sums[i]), int(cnts[i])) == orc.shadow_stats(im), (order, i, im.shape)


# ------------------------------------------------------------------ 2. one pass equals alone
@pytest.mark.parametrize("colors", ["grouped", "one_pass"])
@pytest.mark.parametrize("feats", FEATS, ids=["shapes", "shadows", "both"])
@pytest.mark.parametrize("name", ["alternating", "ladder"])
def test_one_pass_equals_single_images_and_grouped(backend, name, feats, colors):
    imgs = list(_alternating() if name == "alternating" else _ladder())
    with_colors = colors == "one_pass"  # (the colour pass runs beside the shapes pass)
    fs = (("colors",) + feats) if with_colors else feats
    one = backend.process_images(imgs, fs, seed=5, index_base=100, colors=colors, shapes="one_pass")
    grouped = backend.process_images(imgs, fs, seed=5, index_base=100, colors=colors, shapes="grouped")
    alone = _alone(backend, name, imgs, fs, 5, 100)
    off = 0
    for i in range(len(imgs)):
        _same(one[i], alone[i], f"{name} image {i} vs alone", with_colors)
        _same(one[i], grouped[i], f"{name} image {i} vs grouped", with_colors)
        off += len(one[i].shapes)
    if "shapes" not in feats:
        assert off == 0


def test_shape_offsets_are_the_running_sum(backend):
    imgs = list(_alternating())
    n = len(imgs)
    descs, keep, _, _, _ = B._image_descs(imgs, backend.device)
    res = (L.LlfeImageResult * n)()
    shp = (L.LlfeShape * 4096)()
    need = C.c_int64(0)
    rc = backend._lib.llfe_process_images_routes(backend.ctx, descs.ctypes.data, n, L.FEATURE_SHAPES, 0, 5,
                                                 C.c_uint64(5), 100, res, shp, 4096, C.byref(need), None, 0,
                                                 L.IMAGES_SHAPES_ONE_PASS)
    assert rc == L.LLFE_OK
    off = 0
    for i in range(n):
        assert res[i].shape_offset == off
        off += res[i].n_shapes
    assert need.value == off > 0


# ------------------------------------------------------------------ 3. ragged hysteresis
def _check_hysteresis(backend, maps, expected, tile_flags):
    got = backend.hysteresis_images(maps, tile_flags=tile_flags)
    assert len(got) == len(maps)
    for k, ((e, m), (ee, mm)) in enumerate(zip(got, expected)):
        assert np.array_equal(e, ee), (k, maps[k].shape, "edges", tile_flags)
        assert np.array_equal(m, mm), (k, maps[k].shape, "mask", tile_flags)


@pytest.mark.parametrize("tile_flags", [True, False], ids=["flags", "every-tile"])
def test_hysteresis_catalogue_in_one_call(backend, tile_flags):
    maps = [HC.case(name) for name in HC.NAMES]
    _check_hysteresis(backend, maps, [HC.expected(name) for name in HC.NAMES], tile_flags)


@pytest.mark.parametrize("tile_flags", [True, False], ids=["flags", "every-tile"])
def test_hysteresis_catalogue_between_full_and_empty_maps(backend, tile_flags):
    """All-strong and all-weak maps that end exactly on a tile edge (64 x 64) and on a row edge
    (1 x 200) between the cases: with the tight layout their bytes, labels and words lie right
    behind a case's, so a union or a dilation that leaks across an image's edge changes a result."""
    fillers = [np.full(s, v, np.uint8) for s in ((64, 64), (1, 200)) for v in (2, 0)]
    maps, exp = [], []
    for k, name in enumerate(HC.NAMES):
        f = fillers[k % len(fillers)]
        maps += [f, HC.case(name)]
        exp += [HC.reference(f), HC.expected(name)]
    maps.append(fillers[0])
    exp.append(HC.reference(fillers[0]))
    _check_hysteresis(backend, maps, exp, tile_flags)


def test_hysteresis_images_refuses_other_bytes(backend):
    bad = np.ones((5, 9), np.uint8)
    bad[3, 4] = 3
    with pytest.raises(L.LlfeError):
        backend.hysteresis_images([np.ones((4, 4), np.uint8), bad])


# ------------------------------------------------------------------ 4. memory forms
def test_strided_host_and_device_views(backend):
    import torch

    big = synth.synth_numpy(1, 300, 400, seed=4)
    views = [big[10:210, 20:300], big[::1, 50:51], big[150:300, :]]  # row stride 1200 B, 1-column, packed
    dev = torch.from_numpy(big).cuda()
    tviews = [dev[10:210, 20:300], dev[150:300, :]]
    feats = ("shapes", "shadows")
    got = backend.process_images(views + tviews, feats, seed=3, index_base=7, shapes="one_pass")
    ref = [np.ascontiguousarray(v) for v in views] + [np.ascontiguousarray(big[10:210, 20:300]),
                                                      np.ascontiguousarray(big[150:300, :])]
    for i, im in enumerate(ref):
        _same(got[i], backend.process(im[None], feats, seed=3, index_base=7 + i)[0], f"view {i}")


def test_packed_device_images_at_odd_addresses(backend):
    """Packed device images in one buffer from an odd byte on, w % 4 == 0 next to w % 4 != 0, and
    one at an aligned address: the dword paths are chosen per image.  The 25 x 488 image at an
    odd address would have `fast` waves (direct-to-LDS loads) were it aligned; it takes the byte
    path whole."""
    import torch

    a, b, c, d = (synth.synth_numpy(3, 70, 88, seed=12), synth.synth_numpy(4, 64, 65, seed=12),
                  synth.synth_numpy(5, 40, 256, seed=12), synth.synth_numpy(6, 25, 488, seed=12))
    flat = torch.zeros(1 + a.size + b.size + d.size, dtype=torch.uint8, device="cuda")
    flat[1:1 + a.size] = torch.from_numpy(a).reshape(-1).cuda()
    flat[1 + a.size:1 + a.size + b.size] = torch.from_numpy(b).reshape(-1).cuda()
    flat[1 + a.size + b.size:] = torch.from_numpy(d).reshape(-1).cuda()
    va = flat[1:1 + a.size].view(70, 88, 3)
    vb = flat[1 + a.size:1 + a.size + b.size].view(64, 65, 3)
    vc = torch.from_numpy(c).cuda()
    vd = flat[1 + a.size + b.size:].view(25, 488, 3)
    assert va.data_ptr() % 4 == 1 and va.is_contiguous() and vc.data_ptr() % 16 == 0
    assert vd.data_ptr() % 2 == 1 and vd.is_contiguous()
    feats = ("shapes", "shadows")
    got = backend.process_images([va, vb, vc, vd], feats, seed=6, index_base=40, shapes="one_pass")
    for i, im in enumerate((a, b, c, d)):
        _same(got[i], backend.process(im[None], feats, seed=6, index_base=40 + i)[0], f"odd address {i}")
    masks = backend.shape_masks_images([va, vb, vc, vd])
    for m, im in zip(masks, (a, b, c, d)):
        assert np.array_equal(m, backend.shape_mask(im[None])[0].cpu().numpy())


# ------------------------------------------------------------------ 5. launch counts
def test_launch_counts(backend):
    imgs = [synth.synth_numpy(i, 40 + 7 * i, 96 - 5 * i, seed=8) for i in range(8)]
    assert len({im.shape for im in imgs}) == 8
    prev = backend.contour_mode()
    backend.set_contour_mode("host")
    backend.set_profiling(True)
    try:
        added = {}
        for route in ("one_pass", "grouped"):
            before = backend.kernel_stats()
            backend.process_images(imgs, ("shapes", "shadows"), seed=2, index_base=0, shapes=route)
            after = backend.kernel_stats()
            added[route] = {k: after[k]["launches"] - before.get(k, {"launches": 0})["launches"] for k in KERNELS}
    finally:
        backend.set_profiling(False)
        backend.set_contour_mode(prev)
    assert added["one_pass"] == {k: 1 for k in KERNELS}
    assert added["grouped"] == {k: 8 for k in KERNELS}


# ------------------------------------------------------------------ 6. several passes
def test_several_passes_under_a_small_workspace(backend, monkeypatch):
    imgs = list(_ladder())
    feats = ("shapes", "shadows")
    whole = backend.process_images(imgs, feats, seed=13, index_base=60, shapes="one_pass")
    monkeypatch.setenv("LLFE_WORKSPACE_GB", "0.002")
    _, _, passes = B.shapes_images_layout(imgs)
    assert len(passes) >= 2 and sum(p["count"] for p in passes) == len(imgs)
    prev = backend.contour_mode()
    backend.set_contour_mode("host")
    backend.set_profiling(True)
    try:
        before = backend.kernel_stats()
        cut = backend.process_images(imgs, feats, seed=13, index_base=60, shapes="one_pass")
        after = backend.kernel_stats()
        masks = backend.shape_masks_images(imgs)
    finally:
        backend.set_profiling(False)
        backend.set_contour_mode(prev)
    for i in range(len(imgs)):
        _same(cut[i], whole[i], f"pass cut, image {i}")
    assert after["k_stencil"]["launches"] - before.get("k_stencil", {"launches": 0})["launches"] == len(passes)
    monkeypatch.delenv("LLFE_WORKSPACE_GB")
    for m, ref in zip(masks, backend.shape_masks_images(imgs)):
        assert np.array_equal(m, ref)


# ------------------------------------------------------------------ 7. edges of the interface
def test_empty_list_one_image_and_bad_option(backend):
    assert backend.process_images([], ("shapes", "shadows"), shapes="one_pass") == []
    assert backend.shape_masks_images([]) == [] and backend.hysteresis_images([]) == []
    im = synth.synth_numpy(2, 77, 130, seed=5)
    one = backend.process_images([im], ("shapes", "shadows"), seed=1, index_base=9, shapes="one_pass")
    _same(one[0], backend.process(im[None], ("shapes", "shadows"), seed=1, index_base=9)[0], "n = 1")
    with pytest.raises(ValueError):
        backend.process_images([im], ("shapes",), shapes="single")


def test_preprocessing_resize_equals_grouped(backend):
    img = synth.synth_numpy(1, 900, 1500, seed=6)
    small = synth.synth_numpy(0, 120, 200, seed=6)
    feats = ("shapes", "shadows")
    for mode in ("auto", "performance"):  # (only "performance", above 1000 px, resizes the large one)
        one = backend.process_images([img, small], feats, seed=2, index_base=50, preprocessing=mode, shapes="one_pass")
        grouped = backend.process_images([img, small], feats, seed=2, index_base=50, preprocessing=mode)
        for i in range(2):
            _same(one[i], grouped[i], f"{mode} image {i}")
    assert max(one[0].height, one[0].width) == 1000 and (one[1].height, one[1].width) == (120, 200)


def test_short_shape_capacity_through_the_c_entry(backend):
    imgs = list(_alternating())
    n = len(imgs)
    full = backend.process_images(imgs, ("shapes", "shadows"), seed=5, index_base=100, shapes="one_pass")
    total = sum(len(r.shapes) for r in full)
    assert total > 2
    descs, keep, _, _, _ = B._image_descs(imgs, backend.device)
    res = (L.LlfeImageResult * n)()
    shp = (L.LlfeShape * 2)()
    need = C.c_int64(0)
    rc = backend._lib.llfe_process_images_routes(backend.ctx, descs.ctypes.data, n,
                                                 L.FEATURE_SHAPES | L.FEATURE_SHADOWS, 0, 5, C.c_uint64(5), 100, res,
                                                 shp, 2, C.byref(need), None, 0, L.IMAGES_SHAPES_ONE_PASS)
    assert rc == L.LLFE_ERR_CAPACITY and need.value == total
    for i in range(n):  # the records are valid
        assert res[i].n_shapes == len(full[i].shapes) and res[i].n_contours == full[i].n_contours
        assert (res[i].shadow_sum, res[i].shadow_count) == (full[i].shadow_sum, full[i].shadow_count)
    first = [s for r in full for s in r.shapes][:2]
    assert [B._shape_dict(shp[k]) for k in range(2)] == first


def test_invalid_descriptor_names_the_image(backend):
    imgs = [synth.synth_numpy(0, 8, 8, seed=1), synth.synth_numpy(1, 9, 7, seed=1)]
    descs, keep, _, _, _ = B._image_descs(imgs, backend.device)
    descs["row_stride"][1] = 5
    res = (L.LlfeImageResult * 2)()
    rc = backend._lib.llfe_process_images_routes(backend.ctx, descs.ctypes.data, 2, L.FEATURE_SHAPES, 0, 5,
                                                 C.c_uint64(0), 0, res, None, 0, None, None, 0,
                                                 L.IMAGES_SHAPES_ONE_PASS)
    assert rc == L.LLFE_ERR_INVALID
    assert b"image 1" in backend._lib.llfe_last_error(backend.ctx)


def test_gpu_contour_mode_takes_the_grouped_route(backend):
    imgs = list(_alternating())
    feats = ("shapes", "shadows")
    host = backend.process_images(imgs, feats, seed=5, index_base=100, shapes="one_pass")
    prev = backend.contour_mode()
    backend.set_contour_mode("gpu")
    backend.set_profiling(True)
    try:
        before = backend.kernel_stats()
        one = backend.process_images(imgs, feats, seed=5, index_base=100, shapes="one_pass")
        after = backend.kernel_stats()
        grouped = backend.process_images(imgs, feats, seed=5, index_base=100, shapes="grouped")
    finally:
        backend.set_profiling(False)
        backend.set_contour_mode(prev)
    for i in range(len(imgs)):
        _same(one[i], grouped[i], f"gpu contours, image {i} vs grouped")
        _same(one[i], host[i], f"gpu contours, image {i} vs the host pool's one pass")
    # two sizes: two size groups, not one pass
    assert after["k_stencil"]["launches"] - before.get("k_stencil", {"launches": 0})["launches"] == 2


def test_fonts_stay_grouped_beside_the_pass(backend):
    imgs = list(_alternating())[:4]
    feats = ("shapes", "shadows", "fonts")
    one = backend.process_images(imgs, feats, seed=5, index_base=100, shapes="one_pass")
    grouped = backend.process_images(imgs, feats, seed=5, index_base=100)
    for i in range(len(imgs)):
        _same(one[i], grouped[i], f"with fonts, image {i}")
        assert one[i].font == grouped[i].font and one[i].font is not None
