"""The colours of a batch of images of any sizes in one device pass
(process_images(..., colors="one_pass"), color_unique_images): image i's keys equal the
oracle's for its own size and global index, and its result equals a one-image call's and
the size-grouped route's bit for bit, whatever shares the pass with it."""
import functools

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import backend as B
from low_level_feature_extraction_amd import synth

pytestmark = pytest.mark.gpu

FEATS = ("colors", "shapes", "shadows")
KERNELS = ("k_uq_scatter", "k_uq_part", "k_uq_gather", "k_kmeans")
# pixel counts 1, 15, 16, 17, 1023, 1024, 4095, 4096, 4097, 8193, 14400, 14400: the chunk (16),
# wave span (1024) and step (4096) edges of the scatter
LADDER = [(1, 1), (3, 5), (4, 4), (1, 17), (33, 31), (32, 32), (63, 65), (64, 64), (17, 241), (3, 2731), (150, 96),
          (90, 160)]


@functools.lru_cache(maxsize=None)
def _ladder():
    return tuple(synth.synth_numpy(i, h, w, seed=31) for i, (h, w) in enumerate(LADDER))


@functools.lru_cache(maxsize=None)
def _alternating():
    return tuple(synth.synth_numpy(i, (90, 150)[i % 2], (160, 96)[i % 2], seed=21) for i in range(7))


def _same(a, b, tag):  # (tests/test_gpu_ragged.py)
    assert (a.width, a.height, a.n_unique) == (b.width, b.height, b.n_unique), tag
    assert np.array_equal(a.centers_rgb, b.centers_rgb) and np.array_equal(a.counts, b.counts), tag
    assert a.compactness == b.compactness, tag
    assert (a.shadow_sum, a.shadow_count) == (b.shadow_sum, b.shadow_count), tag
    assert a.shapes == b.shapes and a.n_contours == b.n_contours, tag


_ALONE = {}


def _alone(backend, name, imgs, feats, seed, base, n_colors=5):
    """The one-image calls of a list, computed once per (list, features)."""
    key = (name, feats, seed, base, n_colors)
    if key not in _ALONE:
        _ALONE[key] = [backend.process(im[None], feats, seed=seed, index_base=base + i, n_colors=n_colors)[0]
                       for i, im in enumerate(imgs)]
    return _ALONE[key]


# ------------------------------------------------------------------ 1. keys against the oracle
@pytest.mark.parametrize("order", ["input", "reversed"])
def test_keys_equal_the_oracle(backend, orc, order):
    imgs = list(_ladder())
    if order == "reversed":  # the largest images first, the small ones behind long step ranges
        imgs = imgs[::-1]
    got = backend.color_unique_images(imgs, seed=11, index_base=300)
    assert len(got) == len(imgs)
    for i, (im, (keys, nu)) in enumerate(zip(imgs, got)):
        P = im.shape[0] * im.shape[1]
        exp = orc.color_unique(im, orc.device_noise(P, 11, 300 + i))
        assert nu == len(exp), (order, i, im.shape)
        assert np.array_equal(keys, exp), (order, i, im.shape)


# ------------------------------------------------------------------ 2. one pass equals alone
@pytest.mark.parametrize("feats", [("colors",), FEATS], ids=["colors", "three"])
@pytest.mark.parametrize("name", ["alternating", "ladder"])
def test_one_pass_equals_single_images_and_grouped(backend, name, feats):
    imgs = list(_alternating() if name == "alternating" else _ladder())
    one = backend.process_images(imgs, feats, seed=5, index_base=100, colors="one_pass")
    grouped = backend.process_images(imgs, feats, seed=5, index_base=100, colors="grouped")
    alone = _alone(backend, name, imgs, feats, 5, 100)
    for i in range(len(imgs)):
        _same(one[i], alone[i], f"{name} image {i} vs alone")
        _same(one[i], grouped[i], f"{name} image {i} vs grouped")
        assert one[i].palette == grouped[i].palette


# ------------------------------------------------------------------ 3. launch counts
def test_launch_counts(backend):
    imgs = [synth.synth_numpy(i, 40 + 7 * i, 96 - 5 * i, seed=8) for i in range(8)]
    assert len({im.shape for im in imgs}) == 8
    backend.set_profiling(True)
    try:
        added = {}
        for route in ("one_pass", "grouped"):
            before = backend.kernel_stats()
            backend.process_images(imgs, ("colors",), seed=2, index_base=0, colors=route)
            after = backend.kernel_stats()
            added[route] = {k: after[k]["launches"] - before.get(k, {"launches": 0})["launches"] for k in KERNELS}
    finally:
        backend.set_profiling(False)
    assert added["one_pass"] == {k: 1 for k in KERNELS}
    assert added["grouped"] == {k: 8 for k in KERNELS}


# ------------------------------------------------------------------ 4. memory forms
def test_strided_host_and_device_views(backend):
    import torch

    big = synth.synth_numpy(1, 300, 400, seed=4)
    views = [big[10:210, 20:300], big[::1, 50:51], big[150:300, :]]  # row stride 1200 B, 1-column, packed
    dev = torch.from_numpy(big).cuda()
    tviews = [dev[10:210, 20:300], dev[150:300, :]]
    got = backend.process_images(views + tviews, FEATS, seed=3, index_base=7, colors="one_pass")
    ref = [np.ascontiguousarray(v) for v in views] + [np.ascontiguousarray(big[10:210, 20:300]),
                                                      np.ascontiguousarray(big[150:300, :])]
    for i, im in enumerate(ref):
        _same(got[i], backend.process(im[None], FEATS, seed=3, index_base=7 + i)[0], f"view {i}")


def test_packed_device_image_at_an_odd_address(backend):
    import torch

    a, b = synth.synth_numpy(3, 70, 90, seed=12), synth.synth_numpy(4, 64, 64, seed=12)
    flat = torch.zeros(1 + a.size + b.size, dtype=torch.uint8, device="cuda")
    flat[1:1 + a.size] = torch.from_numpy(a).reshape(-1).cuda()
    flat[1 + a.size:] = torch.from_numpy(b).reshape(-1).cuda()
    va = flat[1:1 + a.size].view(70, 90, 3)
    vb = flat[1 + a.size:].view(64, 64, 3)
    assert va.data_ptr() % 16 == 1 and va.is_contiguous()
    got = backend.process_images([va, vb], ("colors",), seed=6, index_base=40, colors="one_pass")
    for i, im in enumerate((a, b)):
        _same(got[i], backend.process(im[None], ("colors",), seed=6, index_base=40 + i)[0], f"odd address {i}")


def test_preprocessing_resize_beside_an_untouched_image(backend):
    from low_level_feature_extraction_amd.utils import preprocess_decoded

    img = synth.synth_numpy(1, 900, 1500, seed=6)
    small = synth.synth_numpy(0, 120, 200, seed=6)
    got = backend.process_images([img, small], FEATS, seed=2, index_base=50, preprocessing="performance",
                                 colors="one_pass")
    pre = preprocess_decoded(img, "performance")
    assert (got[0].height, got[0].width) == pre.shape[:2] and pre.shape[:2] != img.shape[:2]
    _same(got[0], backend.process(np.ascontiguousarray(pre)[None], FEATS, seed=2, index_base=50)[0], "resized")
    _same(got[1], backend.process(small[None], FEATS, seed=2, index_base=51)[0], "small")


# ------------------------------------------------------------------ 5. parity noise
def test_parity_noise_mixed_sizes_vs_oracle(backend, orc):
    from tests import kmeans_bar

    imgs = [synth.synth_numpy(i, (70, 110)[i % 2], (90, 60)[i % 2], seed=9) for i in range(4)]
    noise = [orc.numpy_noise(im.shape[0] * im.shape[1], 60 + i) for i, im in enumerate(imgs)]
    got = backend.process_images(imgs, FEATS, seed=4, index_base=0, noise=noise, colors="one_pass")
    for i, im in enumerate(imgs):
        centers, counts, nu, comp = orc.dominant_colors(im, noise[i], 5, orc.image_rng_state(4, i))
        assert got[i].n_unique == nu
        kmeans_bar.check(got[i].centers_rgb, got[i].counts, got[i].compactness, centers, counts, comp, nu,
                         tag=f"one-pass-{i}")
        assert got[i].shapes == orc.analyze_shapes(im)["shapes"]
        assert (got[i].shadow_sum, got[i].shadow_count) == orc.shadow_stats(im)


def test_parity_noise_for_some_images_only(backend):
    imgs = [synth.synth_numpy(0, 40, 40, seed=1), synth.synth_numpy(1, 30, 50, seed=1)]
    for noise in ([np.zeros(40 * 40 * 3, np.int8), None], [None, np.zeros(30 * 50 * 3, np.int8)]):
        with pytest.raises(L.LlfeError):
            backend.process_images(imgs, ("colors",), noise=noise, colors="one_pass")


# ------------------------------------------------------------------ 6. few colours
def test_flat_and_three_colour_images_among_photos(backend):
    flat = np.full((50, 70, 3), (12, 200, 77), np.uint8)
    three = np.zeros((60, 40, 3), np.uint8)
    three[:20], three[20:40], three[40:] = (250, 10, 10), (10, 250, 10), (10, 10, 250)
    imgs = [synth.synth_numpy(0, 90, 160, seed=3), flat, synth.synth_numpy(1, 64, 64, seed=3), three,
            synth.synth_numpy(2, 150, 96, seed=3)]
    noise = [np.zeros(im.shape[0] * im.shape[1] * 3, np.int8) for im in imgs]
    got = backend.process_images(imgs, ("colors",), seed=9, index_base=20, noise=noise, n_colors=5, colors="one_pass")
    assert (got[1].n_unique, got[3].n_unique) == (1, 3)
    assert (len(got[1].counts), len(got[3].counts)) == (1, 3)
    for i, im in enumerate(imgs):
        one = backend.process(im[None], ("colors",), seed=9, index_base=20 + i, noise=noise[i][None], n_colors=5)[0]
        _same(got[i], one, f"few colours {i}")
        assert got[i].palette == one.palette


# ------------------------------------------------------------------ 7. n_colors = 8
def test_eight_colours_on_three_sizes(backend):
    imgs = [synth.synth_numpy(i, h, w, seed=14) for i, (h, w) in enumerate([(90, 160), (33, 31), (150, 96)])]
    got = backend.process_images(imgs, ("colors",), seed=7, index_base=11, n_colors=8, colors="one_pass")
    for i, im in enumerate(imgs):
        one = backend.process(im[None], ("colors",), seed=7, index_base=11 + i, n_colors=8)[0]
        assert len(one.counts) == 8
        _same(got[i], one, f"K=8 image {i}")


# ------------------------------------------------------------------ 8. several passes
def test_several_passes_under_a_small_workspace(backend, monkeypatch):
    imgs = [synth.synth_numpy(i, 40 + 6 * i, 80 - 4 * i, seed=17) for i in range(7)]
    whole = backend.process_images(imgs, ("colors",), seed=13, index_base=60, colors="one_pass")
    monkeypatch.setenv("LLFE_WORKSPACE_GB", "0.02")
    _, _, passes = B.colors_images_layout(imgs)
    assert len(passes) >= 2 and sum(p["count"] for p in passes) == 7
    backend.set_profiling(True)
    try:
        before = backend.kernel_stats()
        cut = backend.process_images(imgs, ("colors",), seed=13, index_base=60, colors="one_pass")
        after = backend.kernel_stats()
    finally:
        backend.set_profiling(False)
    for i in range(7):
        _same(cut[i], whole[i], f"pass cut, image {i}")
    assert after["k_kmeans"]["launches"] - before.get("k_kmeans", {"launches": 0})["launches"] == len(passes)


# ------------------------------------------------------------------ 9. empty list, bad option
def test_empty_list_and_bad_option(backend):
    assert backend.process_images([], FEATS, colors="one_pass") == []
    assert backend.color_unique_images([]) == []
    with pytest.raises(ValueError):
        backend.process_images([synth.synth_numpy(0, 8, 8, seed=1)], ("colors",), colors="single")
