""""fonts" through the batched pipeline (LLFE_FEATURE_FONTS) and its front-end kernel
k_font_bits, on the GPU.

Expected values always come from the oracle: adaptive_threshold_inv(bgr2gray(img)),
find_contours_external, bounding_rect, then the reference's rules in Python (reference
app/services/analyze/font_detector.py:39-67, 109-155), restated here the way
tests/test_font_detect.py does."""
import asyncio
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import synth
from low_level_feature_extraction_amd.backend import Backend, font_bits_tiling
from low_level_feature_extraction_amd.font_detector import FontDetector

pytestmark = pytest.mark.gpu

FIELDS = ("n_contours", "n_regions", "x", "y", "width", "height", "gray_sum")
SMALL = ((1, 1), (5, 7), (3, 257), (11, 64), (12, 63), (13, 65), (31, 33), (100, 37), (150, 404))


# ------------------------------------------------------------------ the oracle's restatement
def _oracle_record(orc, img):
    binary = orc.adaptive_threshold_inv(orc.bgr2gray(np.ascontiguousarray(img)))
    contours = orc.find_contours_external(np.ascontiguousarray(binary))
    regions = []
    for c in contours:
        x, y, w, h = orc.bounding_rect(c)
        if 0.1 < w / float(h) < 15 and h > 8:
            regions.append((int(x), int(y), int(w), int(h)))
    rec = {"n_contours": len(contours), "n_regions": len(regions), "x": 0, "y": 0, "width": 0, "height": 0,
           "gray_sum": 0}
    if regions:
        x, y, w, h = max(regions, key=lambda r: r[2] * r[3])
        g = orc.bgr2gray(np.ascontiguousarray(img[y:y + h, x:x + w]))
        rec.update(x=x, y=y, width=w, height=h, gray_sum=int(g.sum(dtype=np.uint64)))
    return rec


def _oracle_features(orc, img):
    rec = _oracle_record(orc, img)
    if not rec["n_regions"]:
        return None
    x, y, w, h = rec["x"], rec["y"], rec["width"], rec["height"]
    m = np.mean(orc.bgr2gray(np.ascontiguousarray(img[y:y + h, x:x + w])))
    weight = "Light" if m >= 250 else ("Regular" if m > 190 else "Bold")
    return ("Arial", float(int(h * 0.75)), weight, 0.8)


def _features(f):
    return None if f is None else (f.font_family, f.font_size, f.font_style, f.confidence)


def _same(got, exp, what=""):
    assert got is not None, what
    for f in FIELDS:
        assert got[f] == exp[f], (what, f, got[f], exp[f])


def _glyphs(h, w, seed):
    """dark bars of 4-8 px wide blocks on a light ground, +-3 noise"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), 232, np.uint8)
    for _ in range(7):
        y, x = int(rng.integers(0, h - 24)), int(rng.integers(0, w - 100))
        hh, n = int(rng.integers(10, 20)), int(rng.integers(3, 9))
        for k in range(n):
            bw = int(rng.integers(4, 9))
            x0 = x + k * 11
            img[y:y + hh, x0:x0 + bw] = rng.integers(0, 110)
    return np.clip(img.astype(int) + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)


def _random(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _blocky(n, h, w, seed):
    """random noise with flat dark blocks: regions that pass the font filter at small sizes"""
    rng = np.random.default_rng(seed)
    img = rng.integers(150, 256, (n, h, w, 3), dtype=np.uint8)
    for i in range(n):
        for _ in range(3):
            bh, bw = int(rng.integers(9, max(10, h // 2 + 1))), int(rng.integers(3, max(4, w // 2 + 1)))
            if bh >= h or bw >= w:
                continue
            y, x = int(rng.integers(0, h - bh)), int(rng.integers(0, w - bw))
            img[i, y:y + bh, x:x + bw] = rng.integers(0, 60)
    return img


# ------------------------------------------------------------------ 1. k_font_bits
def _unpack(bits, w):
    """n x h x wpr int64 device tensor -> (n x h x w bool mask, padding bits all zero)"""
    words = bits.cpu().numpy().view(np.uint64)
    n, h, wpr = words.shape
    b = np.unpackbits(words.view(np.uint8).reshape(n, h, wpr * 8), axis=-1, bitorder="little")
    return b[:, :, :w].astype(bool), not b[:, :, w:].any()


def _check_bits(backend, orc, imgs, via=None):
    w = imgs.shape[2]
    got, pad_zero = _unpack(via if via is not None else backend.font_bits(imgs), w)
    assert pad_zero, "bits at x >= w must be zero"
    old = backend.font_binary(imgs).cpu().numpy() != 0
    exp = np.stack([orc.adaptive_threshold_inv(orc.bgr2gray(im)) != 0 for im in imgs])
    assert np.array_equal(old, exp)  # (the path it replaces, for the record)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (imgs.shape, len(bad), bad[:8].tolist())
    assert np.array_equal(got, old)


@pytest.mark.parametrize("h,w", SMALL, ids=[f"{h}x{w}" for h, w in SMALL])
def test_font_bits_small_shapes(backend, orc, h, w):
    _check_bits(backend, orc, _random(2, h, w, 100 * h + w))


def _seam_shape():
    """smallest h x w whose tiling has >= 3 strips and >= 3 segments"""
    strip, _ = font_bits_tiling(1, 1)
    w = 2 * strip + 1
    h = 1
    while -(-h // font_bits_tiling(h, w)[1]) < 3:
        h += 1
    return h, w, strip


def test_font_bits_on_its_seams(backend, orc):
    h, w, strip = _seam_shape()
    seg = font_bits_tiling(h, w)[1]
    assert -(-w // strip) >= 3 and -(-h // seg) >= 3
    _check_bits(backend, orc, _random(2, h, w, 7))
    # image borders one column before / after a strip seam (fewer rows: two segments suffice)
    h2 = seg + 7
    for k in (1, 2):
        for d in (-1, 1):
            _check_bits(backend, orc, _random(2, h2, k * strip + d, 10 * k + d))
    # a smooth image: means near the threshold, long runs of equal bits across the seams
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = ((np.sin(xx / 9.0) + np.cos(yy / 7.0)) * 40 + 128).astype(np.uint8)
    _check_bits(backend, orc, np.stack([np.stack([smooth, smooth // 2 + 60, 255 - smooth], -1)] * 2))


def test_font_bits_through_an_image_table(backend, orc):
    import torch

    imgs = _random(3, 37, 260, 11)
    parts = [torch.from_numpy(im.copy()).to("cuda:0") for im in imgs]  # separately allocated
    _check_bits(backend, orc, imgs, via=backend.font_bits(parts))
    # ... and images whose addresses are not 4-byte aligned (the byte path)
    buf = torch.zeros(3 * 37 * 260 * 3 + 64, dtype=torch.uint8, device="cuda:0")
    odd = []
    for i, im in enumerate(imgs):
        v = buf[i * (37 * 260 * 3 + 3) + 1:][:37 * 260 * 3].view(37, 260, 3)
        v.copy_(torch.from_numpy(im))
        odd.append(v)
    assert any(t.data_ptr() % 4 for t in odd)
    _check_bits(backend, orc, imgs, via=backend.font_bits(odd))


# ------------------------------------------------------------------ 2. fonts only
def _pipeline_images():
    """(name, batch) pairs of one size each"""
    out = [(f"random{h}x{w}", _random(2, h, w, 300 + h + w)) for h, w in SMALL]
    out.append(("blocks", _blocky(3, 60, 90, 2)))
    out.append(("glyphs", np.stack([_glyphs(240, 320, s) for s in range(3)] + [np.full((240, 320, 3), 128, np.uint8)])))
    out.append(("synth", np.stack([synth.synth_numpy(i, 270, 480, seed=5) for i in range(2)])))
    return out


def test_fonts_only_pipeline_matches_the_oracle(backend, orc):
    hits = misses = 0
    for name, imgs in _pipeline_images():
        got = backend.process(imgs, ("fonts",))
        stage = backend.font_detect(imgs)
        for i, im in enumerate(imgs):
            exp = _oracle_record(orc, im)
            _same(got[i].font, exp, (name, i))
            assert got[i].font == stage[i], (name, i)
            hits += exp["n_regions"] > 0
            misses += exp["n_regions"] == 0
    assert hits and misses  # both "has a region" and "none" occurred


# ------------------------------------------------------------------ 3. the other features
def _other_fields(r):
    return (r.centers_rgb.tolist(), r.counts.tolist(), r.n_unique, r.compactness, r.shadow_sum, r.shadow_count,
            r.shapes, r.n_contours, r.width, r.height, r.palette, r.shadow_level)


@pytest.mark.parametrize("mode", ["host", "gpu"])
def test_fonts_leave_the_other_features_alone(backend, orc, mode):
    imgs = np.stack([_glyphs(120, 200, 1), synth.synth_numpy(0, 120, 200, seed=3),
                     synth.synth_numpy(1, 120, 200, seed=3), _blocky(1, 120, 200, 9)[0]])
    before = backend.contour_mode()
    backend.set_contour_mode(mode)
    try:
        three = backend.process(imgs, ("colors", "shapes", "shadows"), seed=17, index_base=40)
        four = backend.process(imgs, ("colors", "shapes", "shadows", "fonts"), seed=17, index_base=40)
        only = backend.process(imgs, ("fonts",), seed=17, index_base=40)
    finally:
        backend.set_contour_mode(before)
    assert any(r.shapes for r in three)
    for i in range(len(imgs)):
        assert _other_fields(four[i]) == _other_fields(three[i]), i
        assert three[i].font is None
        assert four[i].font == only[i].font, i
        _same(four[i].font, _oracle_record(orc, imgs[i]), i)


# ------------------------------------------------------------------ 4. chunking
def test_chunked_batch_gives_the_same_records(backend, orc, monkeypatch):
    imgs = _blocky(5, 48, 80, 21)
    imgs[3] = 200  # one image without a region
    whole = [r.font for r in backend.process(imgs, ("fonts", "shadows"))]
    monkeypatch.setenv("LLFE_WORKSPACE_GB", "0.001")
    assert backend.batch_capacity(48, 80) == 1
    chunked = [r.font for r in backend.process(imgs, ("fonts", "shadows"))]
    assert chunked == whole
    for i, im in enumerate(imgs):
        _same(whole[i], _oracle_record(orc, im), i)
    assert sum(r["n_regions"] > 0 for r in whole) >= 2 and whole[3]["n_regions"] == 0


# ------------------------------------------------------------------ 5. async use
def _records_rc(backend, ticket, n):
    res = (L.LlfeFontResult * max(n, 1))()
    with backend._lock:
        return backend._lib.llfe_font_records(backend.ctx, C.c_int64(ticket), res, n)


def test_two_tickets_in_flight_keep_their_own_records(backend, orc):
    a = np.stack([_glyphs(64, 128, s) for s in range(2)])
    b = _blocky(3, 64, 128, 4)
    ta = backend.submit(a, ("fonts",), seed=1)
    tb = backend.submit(b, ("fonts", "shadows"), seed=1)
    early = (_records_rc(backend, ta, 2), _records_rc(backend, tb, 3))  # not collected yet
    ra = backend.collect(ta)
    mid = (_records_rc(backend, ta, 2), _records_rc(backend, ta, 3), _records_rc(backend, tb, 3))
    rb = backend.collect(tb)
    assert early == (L.LLFE_ERR_INVALID, L.LLFE_ERR_INVALID)
    assert mid == (L.LLFE_OK, L.LLFE_ERR_INVALID, L.LLFE_ERR_INVALID)  # its own; a wrong n; still uncollected
    assert _records_rc(backend, ta, 2) == L.LLFE_ERR_INVALID  # expired with the next collect
    assert _records_rc(backend, tb + 5, 3) == L.LLFE_ERR_INVALID  # unknown
    for i, im in enumerate(a):
        _same(ra[i].font, _oracle_record(orc, im), ("a", i))
    for i, im in enumerate(b):
        _same(rb[i].font, _oracle_record(orc, im), ("b", i))
    # a call without the bit leaves no records
    backend.process(a, ("shadows",))
    assert _records_rc(backend, L.LAST_CALL, 2) == L.LLFE_ERR_INVALID


# ------------------------------------------------------------------ 6. MicroBatcher
def test_submit_images_device_and_host(backend, orc):
    import torch

    imgs = np.stack([_glyphs(64, 160, s) for s in range(3)])
    exp = [_oracle_record(orc, im) for im in imgs]
    before = backend.contour_mode()
    backend.set_contour_mode("host")  # (separately allocated device images are then read in place)
    try:
        dev = [torch.from_numpy(im.copy()).to("cuda:0") for im in imgs]
        got = backend.collect(backend.submit_images(dev, ("fonts",), indices=[5, 6, 7]))
        host = backend.collect(backend.submit_images(list(imgs), ("fonts", "shadows"), indices=[5, 6, 7]))
    finally:
        backend.set_contour_mode(before)
    for i in range(3):
        _same(got[i].font, exp[i], ("device", i))
        _same(host[i].font, exp[i], ("host", i))


def test_micro_batcher_with_fonts(orc):
    from low_level_feature_extraction_amd.batcher import MicroBatcher
    from low_level_feature_extraction_amd.integration import analyze_features

    imgs = [_glyphs(64, 160, 3), np.full((64, 160, 3), 128, np.uint8), synth.synth_numpy(0, 64, 160, seed=2)]
    exp = [_oracle_features(orc, im) for im in imgs]
    assert any(e is None for e in exp) and any(e is not None for e in exp)
    with MicroBatcher(features=("colors", "fonts"), max_batch=8, max_wait_ms=20) as mb:
        async def many():
            return await asyncio.gather(*[mb.analyze(im) for im in imgs])

        res = asyncio.run(many())
        assert [set(r) for r in res] == [{"colors", "fonts"}] * 3
        assert [_features(r["fonts"]) for r in res] == exp
        out = asyncio.run(analyze_features(imgs[0], ["fonts", "text", "colors"], mb))
        assert _features(out[0]) == exp[0] and isinstance(out[1], ValueError)
        assert out[2].metadata["success"] is True


# ------------------------------------------------------------------ 7. ragged list
def test_ragged_list_with_preprocessing(backend, orc):
    rng = np.random.default_rng(8)
    imgs = [_blocky(1, 31, 33, 1)[0], _glyphs(240, 320, 2), synth.synth_numpy(0, 270, 480, seed=4),
            _glyphs(240, 320, 5), _blocky(1, 40, 1100, 6)[0]]
    mode = "performance"
    pre = [orc.preprocess(im, mode) for im in imgs]
    assert pre[4].shape != imgs[4].shape  # the wide one is resized first
    got = backend.process_images(imgs, ("fonts",), preprocessing=mode)
    for i, p in enumerate(pre):
        _same(got[i].font, _oracle_record(orc, np.ascontiguousarray(p)), i)
    assert any(g.font["n_regions"] for g in got)


# ------------------------------------------------------------------ 8. capacity regrowth
def test_contour_capacity_regrowth(orc):
    img = np.full((300, 400, 3), 230, np.uint8)
    img[np.random.default_rng(5).random((300, 400)) < 0.1] = 0
    img[100:112, 50:80] = 0
    exp = _oracle_record(orc, img)
    assert exp["n_contours"] > 5120  # above the default capacity of a one-image pass
    assert (exp["n_regions"], exp["x"], exp["y"], exp["width"], exp["height"]) == (1, 49, 98, 32, 16)
    be = Backend(0)
    try:
        got = be.process(img[None], ("shapes", "fonts"))[0]
    finally:
        be.close()
    _same(got.font, exp)
    assert got.shapes == orc.analyze_shapes(img)["shapes"]


# ------------------------------------------------------------------ 9. too wide for the GPU contour pass
def test_too_wide_image_takes_the_host_path(backend, orc):
    for img in (_random(1, 12, 4100, 13), _blocky(1, 12, 4100, 14)):
        got = backend.process(img, ("fonts",))[0]
        _same(got.font, _oracle_record(orc, img[0]))


# ------------------------------------------------------------------ 10. run_batch
def test_run_batch_returns_font_features(backend, orc):
    from low_level_feature_extraction_amd.pipeline import run_batch

    imgs = np.stack([_glyphs(64, 160, 7), np.full((64, 160, 3), 128, np.uint8)])
    out = run_batch(imgs, ("colors", "fonts"), backend=backend, index_base=0)
    assert [set(o) for o in out] == [{"colors", "fonts"}] * 2
    assert [_features(o["fonts"]) for o in out] == [_features(f) for f in FontDetector.detect_font_batch(imgs)]
    assert [_features(o["fonts"]) for o in out] == [_oracle_features(orc, im) for im in imgs]


# ------------------------------------------------------------------ 11. profiling
def test_profiler_reports_k_font_bits(backend):
    imgs = _random(2, 40, 70, 1)
    backend.set_profiling(True)
    try:
        backend.process(imgs, ("fonts",))
        stats = backend.kernel_stats()
    finally:
        backend.set_profiling(False)
    assert stats.get("k_font_bits", {}).get("launches", 0) >= 1
    assert "k_font_binary" not in stats and "k_font_pack" not in stats  # one kernel, not the pair
