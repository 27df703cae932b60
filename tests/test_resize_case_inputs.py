"""CPU side of tests/resize_cases.py: the tables reach the branches they claim (by the
restatements cv_plan / pil_plan / thumb_plan), the float-box thumbnails stay sensitive to the
box's precision, and the oracle agrees with Pillow itself on every Pillow case and with a second
NumPy statement on the cv2 branches that had none.  The device runs the same cases in
tests/test_gpu_resize_cases.py."""
import numpy as np
import pytest

from tests import resize_cases as RC
from tests.test_text_preprocess import np_otsu, np_resize_cubic


def _plan(c):
    return RC.cv_plan(c.h, c.w, c.cn, c.oh, c.ow, c.interp)


def _diff(got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    return f"{len(bad)} bytes differ, first at {bad[:5].tolist()}" if len(bad) else ""


# --------------------------------------------------------------------------- what the tables reach
def test_cv_cases_reach_every_plan_kind():
    plans = {c: _plan(c) for c in RC.CV_CASES}
    by_group = {}
    for c, p in plans.items():
        by_group.setdefault(c.group, []).append((c, p))
    assert {p.kind for p in plans.values()} == {"COPY", "AREA_FAST", "AREA", "GENERIC"}
    assert all(p.kind == "COPY" for _, p in by_group["copy"])
    assert {c.interp for c, _ in by_group["copy"]} == {"linear", "cubic", "area", "lanczos4"}
    # exact 2x2, as AREA and as LINEAR, for every channel count
    assert all((p.kind, p.fx, p.fy, p.interp) == ("AREA_FAST", 2, 2, "area") for _, p in by_group["fast2x2"])
    assert {c.cn for c, _ in by_group["fast2x2"] if c.interp == "area"} == {1, 2, 3, 4}
    assert {c.cn for c, _ in by_group["fast2x2"] if c.interp == "linear"} >= {2, 3}
    assert sorted((p.kind, p.fx, p.fy) for _, p in by_group["fast"]) == [
        ("AREA_FAST", 3, 2), ("AREA_FAST", 3, 3), ("AREA_FAST", 3, 3), ("AREA_FAST", 9, 7)]
    # 2x in one axis only: LINEAR stays generic
    assert [(p.kind, p.ks, p.interp) for _, p in by_group["one_axis_2x"]] == [("GENERIC", 2, "linear")]
    assert all(p.kind == "AREA" for _, p in by_group["area_tab"])
    ay = {(c.h, c.w): (p.fx, p.fy) for c, p in by_group["area_tab"]}
    assert ay[(9, 7)] == (3.5, 3.0) and 1 < ay[(13, 5)][1] < 1.1 and ay[(1, 9)][1] == 1.0 and ay[(9, 1)][0] == 1.0
    for g, ks, mode in (("generic2", 2, False), ("vec_stop", 2, False), ("area_mode", 2, True), ("generic4", 4, False),
                        ("generic8", 8, False)):
        assert all((p.kind, p.ks, p.area_mode) == ("GENERIC", ks, mode) for _, p in by_group[g]), g
    # every channel count in every kernel
    for kind in ("AREA_FAST", "AREA", "GENERIC"):
        assert {c.cn for c, p in plans.items() if p.kind == kind} == {1, 2, 3, 4}, kind
    for ks in (2, 4, 8):
        assert {c.cn for c, p in plans.items() if p.ks == ks} == {1, 2, 3, 4}, ks


def test_cv_cases_reach_the_vector_stops_and_borders():
    plans = {c: _plan(c) for c in RC.CV_CASES}
    stops = {c.ow * c.cn: (p.x_vec, p.tail) for c, p in plans.items() if c.group == "vec_stop"}
    assert stops == RC.VEC_ROWS
    assert set(stops.values()) >= {(8, 1), (8, 7), (16, 0), (16, 1), (16, 8), (24, 3)} and (0, 6) in stops.values()
    cubic = {(p.x_vec, p.tail) for p in plans.values() if p.ks == 4}
    assert {(0, 9), (0, 10), (0, 15), (48, 3), (48, 4), (16, 8), (16, 4)} <= cubic
    lin = [(c, p) for c, p in plans.items() if p.ks == 2 and not p.area_mode]
    assert any(p.xmin > 0 for _, p in lin) and any(0 < p.xmax < c.ow for c, p in lin)
    assert any(p.xmax == 0 for c, p in lin if c.w == 1) and any(c.h == 1 for c, _ in lin)
    # area_mode: a pure upscale and both mixed directions
    am = sorted((p.fx < 1, p.fy < 1) for c, p in plans.items() if p.area_mode)
    assert (True, True) in am and (True, False) in am and (False, True) in am
    # LANCZOS4: taps clamp on both sides at once (source narrower than the 8 taps), and the two larger shapes
    l4 = [(c, p) for c, p in plans.items() if p.ks == 8]
    assert {c.w for c, _ in l4} >= {1, 2, 3, 5} and {c.h for c, _ in l4} >= {1, 2, 3, 5}
    assert all(p.xmin >= p.xmax for c, p in l4 if c.w < 8)
    assert any(c.oh > c.h and c.w >= 7 for c, _ in l4) and any(c.oh < c.h and c.w >= 8 for c, _ in l4)
    # 1 x 1 outputs and one-pixel sources
    assert any((c.oh, c.ow) == (1, 1) for c in plans) and any((c.h, c.w) == (1, 1) for c in plans)


def test_cv_plan_known_values():
    # (18, 26) -> (7, 13) LINEAR: scale 2, 2.571: no border columns; 39 bytes: 32 + 7
    p = RC.cv_plan(18, 26, 3, 7, 13, "linear")
    assert (p.kind, p.ks, p.xmin, p.xmax, p.x_vec, p.tail) == ("GENERIC", 2, 0, 13, 32, 7)
    # (5, 7) -> (13, 17) LINEAR upscale: fx(0) = 0.5 * 7 / 17 - 0.5 < 0 -> sx = -1 for dx 0 only; sx + 1 >= 7 from dx 16
    p = RC.cv_plan(5, 7, 1, 13, 17, "linear")
    assert (p.xmin, p.xmax, p.x_vec, p.tail) == (1, 16, 16, 1)
    # LANCZOS4 from a 3-pixel row: every column is a border column
    p = RC.cv_plan(3, 3, 4, 7, 8, "lanczos4")
    assert (p.ks, p.xmin, p.xmax) == (8, 8, 0)


def test_exact_2x2_forms_differ_on_the_two_channel_case():
    """(s + 2) >> 2 and the rounded float differ where s % 8 == 2: the cn == 2 image has such cells,
    so taking the shift form there would show."""
    x = RC.images(6, 10, 2)[0].astype(np.int64)
    s = x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2]
    assert (s % 8 == 2).sum() >= 3
    exp = RC.cv_expected(RC.CvCase("fast2x2", 6, 10, 2, 3, 5, "area"))[0]
    assert (exp != ((s + 2) >> 2)).sum() == (s % 8 == 2).sum()


def test_cubic_tie_rows_separate_the_vector_and_tail_forms():
    """Hand-derived ties (resize_cases.cubic_ties): 28.5 and 0.5 round to even in the float form of
    the 16 vector-loop bytes and up in the fixed-point form of the 4 tail bytes."""
    case = next(c for c in RC.CV_CASES if c.group == "cubic_ties")
    p = _plan(case)
    assert (p.kind, p.ks, p.x_vec, p.tail) == ("GENERIC", 4, 16, 4)
    exp = RC.cv_expected(case)[3][:, :, 0]
    assert exp[1].tolist() == [28] * 16 + [29] * 4 and exp[2].tolist() == [0] * 16 + [1] * 4
    assert np.array_equal(exp, np_resize_cubic(RC.cubic_ties()[:, :, 0], 4, 20, 0.5, 0.5))


def test_saturating_images_reach_the_clamps(orc):
    """The 0 / 255 and checkerboard images overshoot: LANCZOS4 and CUBIC results sit on both ends."""
    for c in RC.CV_CASES:
        if c.group in ("generic8", "generic4") and c.h >= 5 and c.w >= 5:
            sat = RC.cv_expected(c)[1]
            assert (sat == 0).any() and (sat == 255).any(), c.id


def test_lanczos_cases_reach_every_arm():
    plans = {c.name: RC.pil_plan(c.h, c.w, c.oh, c.ow, c.box)["f32"] for c in RC.LANCZOS_CASES}
    arms = {n: (p.need_h, p.need_v) for n, p in plans.items()}
    assert arms["both"] == (True, True) and arms["h_only"] == (True, False)
    assert arms["v_only"] == (False, True) and arms["neither"] == arms["neither_full_box"] == (False, False)
    assert (plans["yfirst_h"].yfirst, arms["yfirst_h"]) == (55, (True, True))
    assert (plans["yfirst_no_h"].yfirst, arms["yfirst_no_h"]) == (55, (False, True))
    assert plans["yfirst_h"].ylast == 105 and plans["non_dyadic"].yfirst == 0 and plans["both_ch1"].yfirst == 0
    assert plans["non_dyadic"].bounds_h[0, 0] > 0  # the x box starts inside the row
    assert {c.ch for c in RC.LANCZOS_CASES} == {1, 2, 3, 4}
    assert any((c.oh, c.ow) == (1, 1) for c in RC.LANCZOS_CASES)
    assert any(c.w == 1 for c in RC.LANCZOS_CASES) and any(c.h == 1 for c in RC.LANCZOS_CASES)
    assert any(c.oh > c.h and c.ow > c.w for c in RC.LANCZOS_CASES)


def test_pil_plan_known_values():
    # 4 -> 2 columns, whole row: scale 2, support 6, ksize 13; both windows cover the row
    p = RC.pil_plan(1, 4, 1, 2)["f64"]
    assert p.kk_h.shape == (2, 13) and p.bounds_h.tolist() == [[0, 4], [0, 4]]
    assert p.kk_h.sum(1).tolist() == pytest.approx([1 << 22] * 2, abs=4)
    assert p.kk_h[0, :4].tolist() == p.kk_h[1, 3::-1].tolist()  # mirror images
    assert (p.need_h, p.need_v) == (True, False)
    # a dyadic box gives the same plan at both precisions, w / 3 does not
    assert RC.coeffs_differ(40, 60, 13, 17, (0.0, 0.0, 59.5, 39.25)) == 0
    assert RC.coeffs_differ(334, 217, 200, 100, (0.0, 0.0, 650 / 3, 1300 / 3)) > 0


def test_reduce_cases_cover_the_factors():
    f = {(c.fx, c.fy) for c in RC.REDUCE_CASES}
    assert f >= {(1, 3), (3, 1), (2, 2), (3, 3), (5, 2), (7, 7), (50, 16)}
    for fx, fy in f - {(50, 16), (5, 7)}:
        rem = {(c.w % fx != 0, c.h % fy != 0) for c in RC.REDUCE_CASES if (c.fx, c.fy) == (fx, fy)}
        assert (False, False) in rem and (fx > 1, fy > 1) in rem, (fx, fy)
    assert any(c.fx > c.w and c.fy > c.h for c in RC.REDUCE_CASES)
    assert {c.ch for c in RC.REDUCE_CASES} == {1, 4}
    assert RC.ReduceCase(33, 100, 1, 50, 16) in RC.REDUCE_CASES


def test_thumb_plan_factors_and_sizes(orc):
    from PIL import Image

    for c in RC.THUMB_CASES:
        key = (c.h, c.w, c.max_w, c.max_h)
        p = RC.thumb_plan(c.h, c.w, c.max_w, c.max_h)
        assert (p.fx, p.fy) == RC.THUMB_FACTORS[key], key
        im = Image.new("L", (c.w, c.h))  # (an empty image: the size rule only)
        im.thumbnail((c.max_w, c.max_h), Image.Resampling.LANCZOS)
        assert im.size == (p.ow, p.oh), key
        assert (orc.thumbnail_size(c.w, c.h, c.max_w, c.max_h) or (c.w, c.h)) == (p.ow, p.oh)
        if key in RC.THUMB_SIZES:
            assert (p.oh, p.ow) == RC.THUMB_SIZES[key]
    plans = [RC.thumb_plan(c.h, c.w, c.max_w, c.max_h) for c in RC.THUMB_CASES]
    assert any(not p.resized for p in plans) and any(p.resized and p.box is None for p in plans)
    assert any(p.rem_x and p.rem_y for p in plans) and {c.ch for c in RC.THUMB_CASES} == {1, 3, 4}
    assert RC.thumb_plan(9, 1000, 100, 2)[:2] == (100, 1) and RC.thumb_plan(33, 100, 1, 1)[:2] == (1, 1)
    h, w, mw, mh, seeds = RC.BATCH_CASE
    assert len(seeds) == 3 and all(RC.ThumbCase(h, w, 3, mw, mh, s, True) in RC.THUMB_CASES for s in seeds)


@pytest.mark.parametrize("key", sorted({(c.h, c.w, c.max_w, c.max_h) for c in RC.THUMB_CASES if c.float_box}))
def test_float_box_cases_stay_sensitive(key):
    """Precondition of the float-box thumbnails: the double box and the float32 box give at least
    one different 22-bit coefficient, so a product that takes the box as doubles computes with
    other coefficients than Pillow."""
    h, w, mw, mh = key
    p = RC.thumb_plan(h, w, mw, mh)
    rh, rw = (h + p.fy - 1) // p.fy, (w + p.fx - 1) // p.fx
    assert p.box is not None and RC.coeffs_differ(rh, rw, p.oh, p.ow, p.box) >= 1


# --------------------------------------------------------------------------- oracle against Pillow
@pytest.mark.parametrize("case", RC.LANCZOS_CASES, ids=lambda c: c.id)
def test_oracle_lanczos_vs_pillow(orc, case):
    for kind, x, exp in zip(RC.IMAGE_KINDS, RC.images(case.h, case.w, case.ch), RC.lanczos_expected(case)):
        got = orc.pil_resize_lanczos(x, case.ow, case.oh, case.box)
        assert not _diff(got, exp), (kind, _diff(got, exp))


@pytest.mark.parametrize("case", RC.REDUCE_CASES, ids=lambda c: c.id)
def test_oracle_reduce_vs_pillow(orc, case):
    for kind, x, exp in zip(RC.IMAGE_KINDS, RC.images(case.h, case.w, case.ch), RC.reduce_expected(case)):
        got = orc.pil_reduce(x, case.fx, case.fy)
        assert not _diff(got, exp), (kind, _diff(got, exp))


@pytest.mark.parametrize("case", RC.THUMB_CASES, ids=lambda c: c.id)
def test_oracle_thumbnail_vs_pillow(orc, case):
    """With the box taken as doubles the float-box cases differ from Pillow in isolated bytes
    (5 to 18 per image at these shapes); rounded through float32 they are equal."""
    got = orc.pil_thumbnail(RC.thumb_image(case.h, case.w, case.ch, case.seed), case.max_w, case.max_h)
    d = _diff(got, RC.thumb_expected(case))
    print(case.id, d or "equal")
    assert not d, d


# --------------------------------------------------------------------------- oracle against NumPy
@pytest.mark.parametrize("case", [c for c in RC.CV_CASES if c.interp != "cubic"], ids=lambda c: c.id)
def test_oracle_cv_resize_vs_numpy(case):
    """LINEAR, LANCZOS4 and AREA rows, upscales and area_mode included (CUBIC has np_resize_cubic
    in tests/test_text_preprocess.py)."""
    for kind, x, exp in zip(RC.IMAGE_KINDS, RC.cv_images(case), RC.cv_expected(case)):
        ref = RC.np_cv_resize(x, case.ow, case.oh, case.interp)
        assert not _diff(exp, ref), (kind, _diff(exp, ref))


# --------------------------------------------------------------------------- text
def _gray(img):
    if img.shape[2] == 1:
        return img[:, :, 0]
    b = img.astype(np.uint32)
    return ((b[..., 0] * 1868 + b[..., 1] * 9617 + b[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def test_text_boundary_images_hold_the_counts_stated():
    cases = RC.text_cases()
    for name, ones, inverted in (("ones_2540", 2540, False), ("ones_2541", 2541, True)):
        g = _gray(cases[name])
        assert g.shape == (51, 100) and g.size == 255 * 20
        t = np_otsu(g)
        assert t == 50 and int((g > t).sum()) == ones
        assert (255 * ones > 127 * g.size) == inverted
        out, rt = RC.text_expected(name)
        assert rt == t and np.array_equal(out == 255, (g > t) != inverted)
    assert {cases[n].shape[2] for n in RC.TEXT_NAMES} == {1, 3, 4}


def test_text_cases_reach_what_they_claim(orc):
    cases = RC.text_cases()
    out, t = RC.text_expected("constant")
    assert t == 0 and not out.any()  # one class: every bin skipped; all 255, then inverted
    g = _gray(cases["tie"])
    assert orc.text_size(*g.shape) == g.shape and np_otsu(g) == 10 == RC.text_expected("tie")[1]
    assert set(np.unique(g)) == {10, 200}
    # past one trip of the grid-stride loops, with and without the cubic upscale
    assert cases["second_trip"].shape[:2] == orc.text_size(600, 900) and 600 * 900 > RC.TEXT_GRID
    assert orc.text_size(4, 300) == (100, 7500) and 100 * 7500 > RC.TEXT_GRID
    for name in ("second_trip", "upscaled_second_trip"):
        out, t = RC.text_expected(name)
        assert 0 < t < 255 and 0 < out.mean() <= 127
