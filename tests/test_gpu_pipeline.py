"""GPU parity for the whole hot path and the drop-in services (through the C ABI).

* ``llfe_process_batch`` vs the oracle per image: shadows and shapes bit-exact,
  colours exact in n_unique and within the k-means bar (ΔE76 <= 2.5 after Hungarian
  matching, compactness within 1e-3 relative) in NumPy-noise parity mode.
* seeds are per global image index: results do not depend on batching / sharding.
* Pillow thumbnail (reduce pre-pass + LANCZOS) bit-exact against the golden fixtures
  and Pillow itself (workload sizes; tests/test_gpu_resize_cases.py runs the small
  directed cases of tests/resize_cases.py: boxes, every arm, the float32 thumbnail box).
"""
import dataclasses
import io
import os

import numpy as np
import pytest

from low_level_feature_extraction_amd import synth
from tests.golden.make_golden import REDUCE_CASES
from tests import kmeans_bar
from tests.test_gpu_parity import delta_e_matched

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _batch(n, h, w, seed=0, kind=None):
    return np.stack([synth.synth_numpy(i, h, w, seed=seed, kind=kind) for i in range(n)])


def _check_against_oracle(orc, img, r, noise, seed, index):
    s, c = orc.shadow_stats(img)
    assert (r.shadow_sum, r.shadow_count) == (s, c)
    want_shapes = orc.analyze_shapes(img)["shapes"]
    assert r.shapes == want_shapes
    centers, counts, nu, comp = orc.dominant_colors(img, noise, 5, orc.image_rng_state(seed, index))
    assert r.n_unique == nu
    assert r.centers_rgb.shape == centers.shape
    assert int(r.counts.sum()) == (nu if nu > 1 else len(centers))
    if len(centers) > 1:
        kmeans_bar.check(r.centers_rgb, r.counts, r.compactness, centers, counts, comp, nu,
                         tag=f"pipeline-{img.shape[0]}x{img.shape[1]}")


@pytest.mark.parametrize("h,w,n", [(1, 1, 2), (3, 5, 2), (64, 64, 3), (270, 480, 4), (1080, 1920, 2)])
def test_process_batch_vs_oracle(backend, orc, h, w, n):
    x = _batch(n, h, w, seed=5) if min(h, w) >= 32 else np.random.default_rng(h * w).integers(
        0, 256, (n, h, w, 3), dtype=np.uint8)
    noise = np.stack([orc.numpy_noise(h * w, 300 + i) for i in range(n)])
    seed, base = 77, 1000
    res = backend.process(x, ("colors", "shapes", "shadows"), seed=seed, noise=noise, index_base=base)
    assert len(res) == n
    for i in range(n):
        _check_against_oracle(orc, x[i], res[i], noise[i], seed, base + i)


def test_process_batch_device_input_and_feature_subsets(backend, orc):
    import torch

    x = _batch(3, 180, 320, seed=9)
    xd = torch.from_numpy(x).cuda()
    full = backend.process(xd, ("colors", "shapes", "shadows"), seed=3)
    only_shapes = backend.process(xd, ("shapes",), seed=3)
    only_shadows = backend.process(x, ("shadows",), seed=3)
    only_colors = backend.process(x, ("colors",), seed=3)
    for i in range(3):
        assert full[i].shapes == only_shapes[i].shapes == orc.analyze_shapes(x[i])["shapes"]
        assert (full[i].shadow_sum, full[i].shadow_count) == (only_shadows[i].shadow_sum,
                                                              only_shadows[i].shadow_count)
        assert np.array_equal(full[i].centers_rgb, only_colors[i].centers_rgb)
        assert np.array_equal(full[i].counts, only_colors[i].counts)


def test_results_independent_of_batching(backend):
    """Seeds follow the global image index: one batch of 6 == 2 + 4 with index_base."""
    x = _batch(6, 120, 200, seed=21)
    a = backend.process(x, ("colors",), seed=5, index_base=10)
    b = backend.process(x[:2], ("colors",), seed=5, index_base=10) + backend.process(x[2:], ("colors",), seed=5,
                                                                                       index_base=12)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra.centers_rgb, rb.centers_rgb) and np.array_equal(ra.counts, rb.counts)
        assert ra.n_unique == rb.n_unique and ra.compactness == rb.compactness
    again = backend.process(x, ("colors",), seed=5, index_base=10)
    assert all(np.array_equal(p.centers_rgb, q.centers_rgb) for p, q in zip(a, again))


def _same(a, b):
    for ra, rb in zip(a, b):
        assert np.array_equal(ra.centers_rgb, rb.centers_rgb) and np.array_equal(ra.counts, rb.counts)
        assert ra.n_unique == rb.n_unique and ra.compactness == rb.compactness
        assert ra.shapes == rb.shapes and (ra.shadow_sum, ra.shadow_count) == (rb.shadow_sum, rb.shadow_count)
    assert len(a) == len(b)


def _records_equal(a, b):
    """Every field of two lists of ImageFeatures, arrays by value."""
    assert len(a) == len(b)
    for i, (ra, rb) in enumerate(zip(a, b)):
        for f in dataclasses.fields(ra):
            va, vb = getattr(ra, f.name), getattr(rb, f.name)
            if isinstance(va, np.ndarray):
                assert isinstance(vb, np.ndarray) and va.dtype == vb.dtype and np.array_equal(va, vb), (i, f.name)
            else:
                assert va == vb, (i, f.name)


@pytest.mark.parametrize("mode", ["host", "gpu"])
def test_sync_multi_chunk_matches_whole_batch(backend, monkeypatch, mode):
    """llfe_process_batch over five device passes (one image each: the host result buffers
    alternate while the device workspace stays the same) gives the records of one pass, on
    every field and with all four features, in either contour mode, from a host array and
    from a device tensor."""
    import torch

    feats = ("colors", "shapes", "shadows", "fonts")
    x = _batch(5, 48, 80, seed=13)
    x[3] = 200  # a flat image: no shape, no font region, one colour
    xd = torch.from_numpy(x).cuda()
    prev = backend.contour_mode()
    backend.set_contour_mode(mode)
    try:
        whole = backend.process(x, feats, seed=11, index_base=40)
        _records_equal(backend.process(xd, feats, seed=11, index_base=40), whole)
        monkeypatch.setenv("LLFE_WORKSPACE_GB", "0.001")
        assert backend.batch_capacity(48, 80) == 1
        for src in (x, xd):
            _records_equal(backend.process(src, feats, seed=11, index_base=40), whole)
    finally:
        backend.set_contour_mode(prev)
    assert any(r.shapes for r in whole) and not whole[3].shapes
    assert all(r.font is not None for r in whole)


def test_submit_collect_matches_process(backend):
    """llfe_submit_batch / llfe_collect_batch (two batches in flight) == llfe_process_batch."""
    import torch

    feats = ("colors", "shapes", "shadows")
    x = _batch(5, 150, 260, seed=31)
    y = _batch(3, 97, 131, seed=32)
    xd = torch.from_numpy(x).cuda()
    ref_x = backend.process(x, feats, seed=7, index_base=100)
    ref_y = backend.process(y, feats, seed=8, index_base=200)
    t1 = backend.submit(xd, feats, seed=7, index_base=100)   # device input
    t2 = backend.submit(y, feats, seed=8, index_base=200)    # host input, different size
    _same(backend.collect(t1), ref_x)
    t3 = backend.submit(x, ("shapes",), seed=7, index_base=100)
    _same(backend.collect(t2), ref_y)
    got3 = backend.collect(t3)
    assert [r.shapes for r in got3] == [r.shapes for r in ref_x]
    # a third submission before collecting is refused, and order is enforced
    ta = backend.submit(x, feats, seed=7, index_base=100)
    tb = backend.submit(x, feats, seed=7, index_base=100)
    with pytest.raises(Exception):
        backend.submit(x, feats, seed=7, index_base=100)
    with pytest.raises(Exception):
        backend.collect(tb)
    _same(backend.collect(ta), ref_x)
    _same(backend.collect(tb), ref_x)
    _same(backend.process(x, feats, seed=7, index_base=100), ref_x)  # sync path still fine


def test_three_batches_in_flight(backend):
    """llfe_set_inflight(3): a third workspace; tickets cycle over three slots and still
    match llfe_process_batch, a fourth submission is refused, and the depth only changes
    with nothing in flight."""
    feats = ("colors", "shapes", "shadows")
    xs = [_batch(4, 120 + 10 * j, 200, seed=40 + j) for j in range(3)]
    refs = [backend.process(x, feats, seed=j, index_base=10 * j) for j, x in enumerate(xs)]
    assert backend.inflight == 2
    with pytest.raises(Exception):
        backend.inflight = 4
    backend.inflight = 3
    try:
        tickets = [backend.submit(x, feats, seed=j, index_base=10 * j) for j, x in enumerate(xs)]
        with pytest.raises(Exception):
            backend.submit(xs[0], feats)
        with pytest.raises(Exception):
            backend.inflight = 2
        want = [0, 1, 2]
        for rnd in range(5):  # steady state: slot t % 3 reused with another batch's shape
            _same(backend.collect(tickets.pop(0)), refs[want.pop(0)])
            j = (rnd + 1) % 3
            tickets.append(backend.submit(xs[j], feats, seed=j, index_base=10 * j))
            want.append(j)
        while tickets:
            _same(backend.collect(tickets.pop(0)), refs[want.pop(0)])
    finally:
        backend.inflight = 2
    assert backend.inflight == 2


def test_stage_calls_refused_while_batches_in_flight(backend, orc):
    """Stage entry points share workspace 0 with submitted batches: while a submitted batch
    is uncollected they are refused (no corruption of the batch), afterwards they run."""
    x = _batch(3, 120, 200, seed=61)
    ref = backend.process(x, ("colors", "shapes", "shadows"), seed=4, index_base=50)
    t = backend.submit(x, ("colors", "shapes", "shadows"), seed=4, index_base=50)
    for call in (lambda: backend.color_unique(x, seed=1), lambda: backend.shape_mask(x),
                 lambda: backend.shadow_stats(x), lambda: backend.canny(x),
                 lambda: backend.process_images(list(x), ("shapes",))):
        with pytest.raises(Exception, match="not yet collected"):
            call()
    _same(backend.collect(t), ref)
    assert np.array_equal(backend.shape_mask(x[:1]).cpu().numpy()[0], orc.shape_mask(x[0]))


def test_many_shapes_capacity_retry(backend, orc):
    x = np.zeros((1, 540, 960, 3), np.uint8)
    for y in range(6, 530, 24):  # a grid of separated 12 x 12 squares -> ~880 shapes
        for xx in range(6, 950, 24):
            x[0, y:y + 12, xx:xx + 12] = (200, 180, 40)
    r = backend.process(x, ("shapes",))[0]
    assert r.shapes == orc.analyze_shapes(x[0])["shapes"]
    assert len(r.shapes) > 64  # more than the binding's initial per-image capacity


def test_n_colors_parameter(backend, orc):
    x = _batch(2, 96, 128, seed=2)
    noise = np.stack([orc.numpy_noise(96 * 128, i) for i in range(2)])
    for k in (2, 3, 4, 5):
        res = backend.process(x, ("colors",), seed=1, noise=noise, n_colors=k)
        for i, r in enumerate(res):
            centers, counts, nu, comp = orc.dominant_colors(x[i], noise[i], k, orc.image_rng_state(1, i))
            assert len(r.centers_rgb) == len(centers) == min(k, nu)
            assert delta_e_matched(r.centers_rgb, centers) <= 2.5


def test_n_colors_below_five_on_cell_tables(backend, orc):
    """K in {1, 2, 3, 4} on a photo-class 1080p image: its cube table has >= 8192 cubes, so
    both k-means++ and Lloyd take the 4 x 8 x 8 cell path with unused centres (the -inf
    margins / +inf forms of centres k >= K), compared with the oracle on the k-means bar
    (the served tests only reach the cell path at K = 5)."""
    x = synth.synth_numpy(1, 1080, 1920, seed=91, kind="photo")[None]
    noise = orc.numpy_noise(1080 * 1920, 7)[None]
    for k in (1, 2, 3, 4):
        r = backend.process(x, ("colors",), seed=3, noise=noise, n_colors=k)[0]
        centers, counts, nu, comp = orc.dominant_colors(x[0], noise[0], k, orc.image_rng_state(3, 0))
        assert nu > 300_000  # photo class: ~34k occupied 4 x 4 x 4 cubes, >= the cell path's 8192
        assert r.n_unique == nu and len(r.centers_rgb) == len(centers)
        if k == 1:  # no k-means (color_extractor.py:185-186): the first unique colours, counts [U, 0, ...]
            assert np.array_equal(np.asarray(r.centers_rgb), np.asarray(centers))
            assert np.array_equal(np.asarray(r.counts), np.asarray(counts))
            continue
        assert len(centers) == k
        assert int(np.sum(r.counts)) == nu
        kmeans_bar.check(r.centers_rgb, r.counts, r.compactness, centers, counts, comp, nu, tag=f"cells-K{k}")


@pytest.mark.parametrize("k", [6, 8, 12, 32])
def test_n_colors_above_five_vs_oracle(backend, orc, k):
    """K = min(n_colors, U) > 5 runs the general-K kernel (kmeans_big.hip): same attempts
    and the same bar as K <= 5, through the batch path and the fine-grained llfe_kmeans."""
    import torch

    x = np.stack([synth.synth_numpy(i, 120, 200, seed=31) for i in range(2)])
    noise = np.stack([orc.numpy_noise(120 * 200, 40 + i) for i in range(2)])
    res = backend.process(x, ("colors",), seed=6, noise=noise, n_colors=k)
    for i, r in enumerate(res):
        centers, counts, nu, comp = orc.dominant_colors(x[i], noise[i], k, orc.image_rng_state(6, i))
        assert len(r.centers_rgb) == len(centers) == min(k, nu)
        assert int(np.sum(r.counts)) == nu
        kmeans_bar.check(r.centers_rgb, r.counts, r.compactness, centers, counts, comp, nu, tag=f"batch-K{k}")
    keys_list = [orc.color_unique(x[i], noise[i]) for i in range(2)]
    stride = (max(len(q) for q in keys_list) + 3) // 4 * 4
    buf = np.zeros((2, stride), np.uint32)
    for i, q in enumerate(keys_list):
        buf[i, : len(q)] = q
    got = backend.kmeans(torch.from_numpy(buf.view(np.int32)).cuda(), np.array([len(q) for q in keys_list]), k, seed=9)
    for i, q in enumerate(keys_list):
        data = np.stack([(q >> 16) & 255, (q >> 8) & 255, q & 255], -1).astype(np.float32)
        comp, labels, centers, counts, _ = orc.kmeans(data, min(k, len(q)), rng_state=orc.image_rng_state(9, i))
        gc, gcount, gcomp = got[i]
        kmeans_bar.check(gc, gcount, gcomp, centers.astype(np.uint8), np.bincount(labels, minlength=len(centers)),
                         comp, len(q), tag=f"abi-K{k}")


def test_n_colors_above_five_few_unique(backend, orc):
    """U < n_colors: K = U (every colour its own cluster)."""
    x = np.zeros((1, 30, 40, 3), np.uint8)
    x[0, :, :20] = (10, 200, 30)
    x[0, :10, 20:] = (90, 20, 240)
    x[0, 10:, 20:] = (250, 250, 5)
    noise = np.zeros((1, 30 * 40 * 3), np.int8)
    r = backend.process(x, ("colors",), seed=2, noise=noise, n_colors=12)[0]
    centers, counts, nu, comp = orc.dominant_colors(x[0], noise[0], 12, orc.image_rng_state(2, 0))
    assert nu == 3 and len(r.centers_rgb) == 3
    kmeans_bar.check(r.centers_rgb, r.counts, r.compactness, centers, counts, comp, nu, tag="K12-U3")


# --------------------------------------------------------------------------- drop-ins
def test_shape_and_shadow_analyzers(orc):
    from low_level_feature_extraction_amd import ShadowAnalyzer, ShapeAnalyzer

    for i in range(3):
        img = synth.synth_numpy(i, 270, 480, seed=13)
        assert ShapeAnalyzer.analyze_shapes(img) == orc.analyze_shapes(img)
        assert ShadowAnalyzer.analyze_shadow_level(img) == orc.analyze_shadow_level(img)
        assert np.array_equal(ShapeAnalyzer.preprocess_image(img), orc.shape_mask(img))
        assert np.array_equal(ShadowAnalyzer.preprocess_image(img), orc.blur5(orc.bgr2gray(img)))


def test_color_extractor_dropin(orc):
    from PIL import Image

    from low_level_feature_extraction_amd import ColorExtractor

    img = synth.synth_numpy(1, 120, 160, seed=3)
    for k in (1, 2, 5):
        res = ColorExtractor.extract_colors(img, n_colors=k)
        assert res.metadata["success"] is True, res.metadata
        assert len(res.accent) == 3
    res = ColorExtractor.extract_colors(Image.fromarray(img[:, :, ::-1]))
    assert res.metadata["success"] is True
    res = ColorExtractor.extract_colors(np.zeros((2, 5, 6, 3), np.uint8))  # 4-D: flattened like the reference
    assert res.metadata["success"] is True
    assert ColorExtractor.extract_colors(img, n_colors=9).metadata["success"] is True  # general-K kernel
    assert ColorExtractor.extract_colors(img, n_colors=33).metadata["success"] is False  # > LLFE_MAX_COLORS
    batch = ColorExtractor.extract_colors_batch([img, img[:50], img], seed=4)
    assert len(batch) == 3 and all(b.metadata["success"] for b in batch)


def test_run_batch_mixed_sizes_matches_single_batches(backend):
    from low_level_feature_extraction_amd.pipeline import run_batch

    imgs = [synth.synth_numpy(i, 64 + 32 * (i % 2), 96, seed=8) for i in range(5)]
    got = run_batch(imgs, ("colors", "shapes", "shadows"), seed=9, raw=True)
    assert [r.height for r in got] == [im.shape[0] for im in imgs]  # input order kept across size groups
    for im, r in zip(imgs, got):
        one = backend.process(im[None], ("shapes", "shadows"), seed=9)[0]
        assert r.shapes == one.shapes and (r.shadow_sum, r.shadow_count) == (one.shadow_sum, one.shadow_count)


# --------------------------------------------------------------------------- Pillow resize path
@pytest.mark.parametrize("k", range(len(REDUCE_CASES)))
def test_reduce_vs_golden(backend, k):
    h, w, fx, fy = REDUCE_CASES[k]
    a = np.random.default_rng(2000 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = np.load(os.path.join(GOLD, "pil_reduce.npz"))[f"case{k}"]
    assert np.array_equal(backend.reduce_pil(a, fx, fy).cpu().numpy(), want)


def test_thumbnail_reduce_prepass_vs_golden(backend):
    a = np.random.default_rng(77).integers(0, 256, (90, 200, 3), dtype=np.uint8)
    want = np.load(os.path.join(GOLD, "pil_lanczos.npz"))["thumb_reduce"]
    assert np.array_equal(backend.thumbnail_pil(a, 40, 20).cpu().numpy(), want)


@pytest.mark.parametrize("h,w", [(2160, 3840), (4320, 7680), (1125, 2000), (4000, 1000), (300, 9000), (1081, 1919)])
def test_thumbnail_vs_pillow(backend, orc, h, w):
    from PIL import Image

    a = np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    im = Image.fromarray(a)
    im.thumbnail((1920, 1080), Image.Resampling.LANCZOS)
    want = np.array(im)
    got = backend.thumbnail_pil(a).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


def test_auto_process_image_dropin():
    from PIL import Image

    from low_level_feature_extraction_amd import ImageProcessor

    rgb = np.random.default_rng(1).integers(0, 256, (2160, 3840, 3), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG")
    out = ImageProcessor.auto_process_image(buf.getvalue())
    im = Image.fromarray(rgb)
    im.thumbnail((1920, 1080), Image.Resampling.LANCZOS)
    assert np.array_equal(out, np.array(im)[:, :, ::-1])
    small = io.BytesIO()
    Image.fromarray(rgb[:100, :100]).save(small, format="PNG")
    assert np.array_equal(ImageProcessor.auto_process_image(small.getvalue()), rgb[:100, :100, ::-1])
    with pytest.raises(ValueError):
        ImageProcessor.auto_process_image(b"junk")



@pytest.mark.parametrize("h,w", [(2160, 3840), (1500, 1000), (5000, 2400)])
def test_thumbnail_batch_vs_pillow(backend, h, w):
    """llfe_thumbnail_pil_batch (one launch sequence for the batch) equals Pillow per image,
    including the reduce() pre-pass (5000 x 2400)."""
    from PIL import Image

    a = np.random.default_rng(h * 3 + w).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    got = backend.thumbnail_pil_batch(a).cpu().numpy()
    for i in range(3):
        im = Image.fromarray(a[i])
        im.thumbnail((1920, 1080), Image.Resampling.LANCZOS)
        assert np.array_equal(got[i], np.array(im)), i


def test_auto_process_images_batched():
    from PIL import Image

    from low_level_feature_extraction_amd import ImageProcessor

    rng = np.random.default_rng(2)
    rgbs = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(2160, 3840, 3), (300, 200, 3), (2160, 3840, 3),
                                                                  (1200, 2500, 3)]]
    blobs = []
    for x in rgbs:
        buf = io.BytesIO()
        Image.fromarray(x).save(buf, format="PNG")
        blobs.append(buf.getvalue())
    blobs.insert(2, b"junk")
    out = ImageProcessor.auto_process_images(blobs)
    assert isinstance(out[2], ValueError)
    got = [o for j, o in enumerate(out) if j != 2]
    for x, g in zip(rgbs, got):
        im = Image.fromarray(x)
        im.thumbnail((1920, 1080), Image.Resampling.LANCZOS)
        assert np.array_equal(g, np.array(im)[:, :, ::-1])


# --------------------------------------------------------------------------- cv2.resize modes
# validate_and_preprocess_image (utils.py:118-143): the GPU resize (llfe_resize_cv) against
# the oracle's OpenCV restatement, bit-exact.  Sizes cover AREA 2x / 3x (resizeAreaFast_),
# fractional AREA (resizeArea_), LINEAR (incl. the exact-2x -> AREA rule and the vector /
# scalar vertical split), LANCZOS4, grey and 4-channel images.
CV_RESIZE_CASES = [
    (3000, 4000, 1500, 2000, "area"), (1440, 2560, 1125, 2000, "area"), (2400, 6000, 800, 2000, "area"),
    (1080, 1920, 562, 1000, "linear"), (2000, 1500, 1000, 750, "linear"), (1201, 1333, 900, 1000, "linear"),
    (4000, 6000, 2666, 4000, "lanczos4"), (4500, 4100, 4000, 3644, "lanczos4"), (97, 131, 40, 57, "lanczos4"),
    (97, 131, 40, 57, "area"), (97, 131, 40, 57, "linear"), (9, 7, 3, 2, "area"),
]


@pytest.mark.parametrize("h,w,oh,ow,interp", CV_RESIZE_CASES)
def test_cv_resize_vs_oracle(backend, orc, h, w, oh, ow, interp):
    rng = np.random.default_rng(h * 31 + w)
    img = synth.synth_numpy(3, h, w, seed=5, kind="photo") if h * w > 10000 else rng.integers(
        0, 256, (h, w, 3), dtype=np.uint8)
    got = backend.resize_cv(img, ow, oh, interp).cpu().numpy()
    exp = orc.cv_resize(img, ow, oh, interp)
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), int((got != exp).sum())


@pytest.mark.parametrize("ch", [1, 4])
def test_cv_resize_channels(backend, orc, ch):
    img = np.random.default_rng(ch).integers(0, 256, (333, 517, ch), dtype=np.uint8)
    for interp, (ow, oh) in [("area", (200, 129)), ("linear", (250, 161)), ("lanczos4", (300, 193)),
                             ("area", (172, 111))]:
        got = backend.resize_cv(img if ch > 1 else img[:, :, 0], ow, oh, interp).cpu().numpy()
        exp = orc.cv_resize(img if ch > 1 else img[:, :, 0], ow, oh, interp)
        assert np.array_equal(got, exp), (interp, int((got != exp).sum()))


def test_validate_and_preprocess_image_resizes_on_gpu(orc):
    import asyncio

    from PIL import Image

    from low_level_feature_extraction_amd.utils import validate_and_preprocess_image

    rgb = synth.synth_numpy(1, 1300, 2200, seed=3)[:, :, ::-1].copy()
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG")
    bgr = rgb[:, :, ::-1]
    for mode in ("auto", "performance", "high_quality", "none"):
        out = asyncio.run(validate_and_preprocess_image(buf.getvalue(), "r", mode))
        assert np.array_equal(out, orc.preprocess(np.ascontiguousarray(bgr), mode)), mode


def _flat(h, w, colours, seed=0):
    """Image made of vertical bands of the given BGR colours (few unique colours)."""
    img = np.zeros((h, w, 3), np.uint8)
    bands = np.array_split(np.arange(w), len(colours))
    for c, xs in zip(colours, bands):
        img[:, xs] = c
    return img


@pytest.mark.parametrize("ncol", [1, 2, 3, 5, 6, 9])
def test_few_unique_colours_vs_oracle(backend, orc, ncol):
    """U <= 5 (K = U: every colour its own centre, compactness 0), U = 1 (K = 1) and a few
    more colours than K, with zero parity noise so U is exactly the band count."""
    rng = np.random.default_rng(ncol)
    cols = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(ncol)]
    x = np.stack([_flat(90, 160, cols), _flat(90, 160, cols[::-1])])
    noise = np.zeros((2, 90 * 160 * 3), np.int8)
    res = backend.process(x, ("colors", "shapes", "shadows"), seed=3, noise=noise, index_base=40)
    for i, r in enumerate(res):
        _check_against_oracle(orc, x[i], r, noise[i], 3, 40 + i)
        assert r.n_unique == ncol
        if ncol <= 5:
            got = sorted(map(tuple, r.centers_rgb.tolist()))
            want = sorted((c[2], c[1], c[0]) for c in cols)  # BGR bands -> RGB centres
            assert got == want and r.compactness == 0.0


def test_empty_batch(backend):
    assert backend.process(np.zeros((0, 32, 48, 3), np.uint8)) == []
    t = backend.submit(np.zeros((0, 32, 48, 3), np.uint8))
    assert backend.collect(t) == []


def test_backend_before_torch_in_a_fresh_process():
    # libllfe and PyTorch-ROCm each load a HIP runtime: a Backend created before any
    # torch call must still leave torch's device usable (Backend initialises it first)
    import subprocess
    import sys

    code = ("import numpy as np\n"
            "from low_level_feature_extraction_amd.backend import Backend\n"
            "be = Backend.get(0)\n"
            "keys, nu = be.color_unique(np.zeros((1, 8, 8, 3), np.uint8), noise=np.zeros(192, np.int8))\n"
            "print(int(nu[0]))\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "1"


def test_kernel_stats_cover_stage_entry_points(backend):
    """Profiling records of the fine-grained entry points (here llfe_color_unique, which
    never waits on its stream) reach llfe_kernel_stats once their launches completed."""
    import torch

    x = _batch(3, 96, 128, seed=5)
    backend.set_profiling(True)
    try:
        keys, nu = backend.color_unique(x, seed=1)
        torch.cuda.synchronize()
        st = backend.kernel_stats()
        for name in ("k_uq_scatter", "k_uq_part", "k_uq_gather"):
            assert st[name]["launches"] >= 1 and st[name]["total_ms"] > 0, (name, st)
        assert "k_uq_hist" not in st  # (no histogram pass: the scatter writes step segments)
    finally:
        backend.set_profiling(False)
