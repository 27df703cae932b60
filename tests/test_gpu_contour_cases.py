"""The GPU contour path (csrc/contours_gpu.hip) on the directed masks of tests/contour_cases.py.

Every case goes through the three entries of the path and is compared bit for bit:

* ``find_contours_gpu``: the contour list, order and vertices, vs ``orc.find_contours_external``;
* ``shapes_from_masks_gpu``: the shape records and ``n_contours`` vs ``orc.classify_contour`` over
  those contours (the full mode: k_ct_trace<false>, k_ct_scan<false>, k_ct_bases, k_ct_shapes);
* ``font_detect(None, binary=mask, regions=True)``: ``n_contours``, the region list and the largest
  region vs the same contours under the rule of tests/test_font_detect.py (the boxes-only mode).

tests/test_contour_case_inputs.py asserts, without a GPU, that each mask reaches the branch it is
named for; the table of cases is in tests/contour_cases.py.
"""
import numpy as np
import pytest

from tests import contour_cases as cc

pytestmark = pytest.mark.gpu


def _font_record(orc, contours):
    """llfe_font_detect's record for a binary with these external contours and no image: the
    rule of tests/test_font_detect.py::_oracle_record (font_detector.py:39-67, 109-155)."""
    regions = []
    for c in contours:
        x, y, w, h = orc.bounding_rect(c)
        if 0.1 < w / float(h) < 15 and h > 8:
            regions.append((int(x), int(y), int(w), int(h)))
    rec = {"n_contours": len(contours), "n_regions": len(regions), "x": 0, "y": 0, "width": 0, "height": 0,
           "gray_sum": 0, "regions": regions}
    if regions:
        x, y, w, h = max(regions, key=lambda r: r[2] * r[3])
        rec.update(x=x, y=y, width=w, height=h)
    return rec


def _shapes(orc, contours):
    return [s for s in (orc.classify_contour(c) for c in contours) if s is not None]


@pytest.fixture(scope="module")
def expected(orc):
    """name -> (contours, shape records, font record) of a case from the oracle, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            cs = orc.find_contours_external(cc.SINGLE[name]())
            cache[name] = (cs, _shapes(orc, cs), _font_record(orc, cs))
        return cache[name]

    return get


def _check_contours(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: contour {k}")


# ------------------------------------------------------------------ every single mask, three entries
@pytest.mark.parametrize("name", sorted(cc.SINGLE))
def test_find_contours_gpu_on_case(backend, expected, name):
    _check_contours(backend.find_contours_gpu(cc.SINGLE[name]()), expected(name)[0], name)


@pytest.mark.parametrize("name", sorted(cc.SINGLE))
def test_shapes_from_masks_gpu_on_case(backend, expected, name):
    cs, shapes, _ = expected(name)
    got, ncont = backend.shapes_from_masks_gpu(cc.SINGLE[name]()[None])
    assert ncont[0] == len(cs)
    assert got[0] == shapes
    if name in cc.COMBS or name in ("spiral", "diagonal", "staircase", "window_edge"):
        assert len(shapes) == 1     # the long border is a kept shape: its geometry was computed


@pytest.mark.parametrize("name", sorted(cc.SINGLE))
def test_font_detect_binary_on_case(backend, expected, name):
    want = expected(name)[2]
    (got,) = backend.font_detect(None, binary=cc.SINGLE[name](), regions=True)
    assert got == want


# ------------------------------------------------------------------ same shape, one batch
def test_cases_of_one_shape_in_one_batch(backend, expected):
    """One wave of k_ct_scan per image: the LDS state of one image (its rejection boxes) must not
    leak into its neighbours, and the refs and shapes of several images share the pools."""
    names = ["rej_grid", "rej_64", "rej_straddle_many", "rej_65", "rej_66", "rej_straddle_few"]
    masks = np.stack([cc.SINGLE[n]() for n in names])
    got, ncont = backend.shapes_from_masks_gpu(masks)
    fonts = backend.font_detect(None, binary=masks, regions=True)
    for i, n in enumerate(names):
        cs, shapes, font = expected(n)
        assert ncont[i] == len(cs) and got[i] == shapes, n
        assert fonts[i] == font, n


# ------------------------------------------------------------------ B5
@pytest.mark.parametrize("ph,pw", [(3, 4), (4, 3)])
def test_every_pattern_over_a_tile_corner(backend, orc, ph, pw):
    """4096 images in one call: the border unions over the corner of four tiles in every
    configuration of ph x pw pixels, and k_ct_bases' carry over four 1024-image chunks (every
    image keeps one shape, whose width depends on the image index)."""
    masks = cc.corners(ph, pw)
    want = [orc.find_contours_external(m) for m in masks]
    got, ncont = backend.shapes_from_masks_gpu(masks)
    fonts = backend.font_detect(None, binary=masks, regions=True)
    bad = [i for i in range(len(masks)) if ncont[i] != len(want[i])]
    assert not bad, (len(bad), bad[:8])
    bad = [i for i in range(len(masks)) if fonts[i]["n_contours"] != len(want[i])]
    assert not bad, (len(bad), bad[:8])
    for i in range(len(masks)):
        if got[i] != _shapes(orc, want[i]) or fonts[i] != _font_record(orc, want[i]):
            raise AssertionError(f"image {i}: {got[i]} / {fonts[i]}")
    assert sum(len(g) for g in got) == len(masks)


# ------------------------------------------------------------------ B9
def test_vertex_pool_regrowth_then_a_small_mask(orc, expected):
    """87 930 vertices in one call, above the default pool of 1 * 16384 + 65536: k_ct_trace flags
    kCtOverflowPts, the host grows the pool and runs the pass again.  A fresh context, so that
    no earlier test has grown it; the same context must then still be right on small masks."""
    from low_level_feature_extraction_amd.backend import Backend

    be = Backend(0)
    try:
        cs, shapes, font = expected("regrow")
        _check_contours(be.find_contours_gpu(cc.regrow()), cs, "regrow")
        for name in ("rej_66", "comb_b", "corner_ne_33x65"):
            cs, shapes, font = expected(name)
            m = cc.SINGLE[name]()
            _check_contours(be.find_contours_gpu(m), cs, name)
            got, ncont = be.shapes_from_masks_gpu(m[None])
            assert ncont[0] == len(cs) and got[0] == shapes, name
            assert be.font_detect(None, binary=m, regions=True)[0] == font, name
    finally:
        be.close()
