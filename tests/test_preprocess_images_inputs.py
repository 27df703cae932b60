"""CPU checks for llfe_preprocess_images / llfe_resize_cv_images: the case tables of
tests/preprocess_images_cases.py reach the plans they claim (resize_cases.cv_plan, the restatement
of cv_resize_plan), the host-only half of the ABI (the layout, the tiling query, argument checks)
behaves as include/llfe.h says, and a second NumPy statement of cv2.resize agrees with the oracle
on every case.  The device half is tests/test_gpu_preprocess_images.py."""
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import backend as B
from tests import preprocess_images_cases as PC
from tests import resize_cases as RC

PRE = {"none": 0, "auto": 1, "high_quality": 2, "performance": 3}


def _layout(images, mode):
    descs, keep, _, _, _ = B._image_descs(images, 0)
    outs = (L.LlfeResizeOut * max(len(keep), 1))()
    total = C.c_int64(-1)
    rc = L.lib().llfe_preprocess_images_layout(descs.ctypes.data, len(keep), mode, outs, C.byref(total))
    return rc, outs, total.value


@pytest.mark.parametrize("c", PC.RULE_CASES, ids=lambda c: c.id)
def test_table_matches_the_rule_and_the_plan(c):
    r = PC.rule(c.h, c.w, c.mode)
    if not c.resized:
        assert r is None and c.kind == "COPY"
        return
    assert r == (c.oh, c.ow, c.interp)
    assert B.preprocess_size(c.w, c.h, c.mode) == (c.ow, c.oh, PC.CODE[c.interp])
    p = RC.cv_plan(c.h, c.w, 3, c.oh, c.ow, c.interp)
    assert p.kind == c.kind
    for k, v in c.facts.items():
        got = getattr(p, k)
        assert got == pytest.approx(v, rel=1e-12) if isinstance(v, float) else got == v, (k, got, v)
    if c.kind == "AREA":
        assert p.fx >= 1 and p.fy >= 1 and not (float(p.fx).is_integer() and float(p.fy).is_integer())
    if c.facts.get("ks") == 8 and c.w == 12:
        assert p.xmin == 3 and p.xmax == 6 < c.ow  # the taps clamp on both sides


@pytest.mark.parametrize("mode", PC.MODES)
def test_layout_follows_the_rule_aligned_and_packed(mode):
    cases = PC.rule_cases(mode)
    imgs, exp = PC.rule_batch(mode)
    rc, outs, total = _layout(imgs, PRE[mode])
    assert rc == L.LLFE_OK
    end = 0
    for c, e, o in zip(cases, exp, outs):
        assert (o.height, o.width) == e.shape[:2] == (c.oh, c.ow), c.id
        assert o.resized == int(c.resized) and o.interpolation == (PC.CODE[c.interp] if c.resized else 0), c.id
        assert o.offset % 16 == 0 and 0 <= o.offset - end < 16, c.id  # input order, only the alignment gap
        end = o.offset + o.height * o.width * 3
    assert total == end
    lay, tot = B.preprocess_images_layout(imgs, mode)
    assert tot == total
    assert lay == [(o.offset, o.height, o.width, o.interpolation, o.resized) for o in outs[:len(cases)]]


def test_mode_none_leaves_every_image():
    imgs = [PC.image(6, 4000), PC.image(9, 4032, 1)]
    rc, outs, total = _layout(imgs, PRE["none"])
    assert rc == L.LLFE_OK
    assert [(o.height, o.width, o.interpolation, o.resized) for o in outs] == [(6, 4000, 0, 0), (9, 4032, 0, 0)]


def test_layout_of_an_empty_batch():
    total = C.c_int64(-1)
    assert L.lib().llfe_preprocess_images_layout(None, 0, 1, None, C.byref(total)) == L.LLFE_OK
    assert total.value == 0
    assert B.preprocess_images_layout([], "auto") == ([], 0)


def test_layout_rejects_bad_arguments():
    lib = L.lib()
    img = np.zeros((8, 9, 3), np.uint8)
    descs, keep, _, _, _ = B._image_descs([img, img], 0)
    outs = (L.LlfeResizeOut * 2)()
    total = C.c_int64(0)
    ok = lambda d=descs, n=2, m=1, o=outs, t=C.byref(total): lib.llfe_preprocess_images_layout(
        d.ctypes.data if d is not None else None, n, m, o, t)
    assert ok() == L.LLFE_OK
    assert ok(n=-1) == L.LLFE_ERR_INVALID
    assert ok(o=None) == L.LLFE_ERR_INVALID
    assert ok(t=None) == L.LLFE_ERR_INVALID
    assert ok(d=None) == L.LLFE_ERR_INVALID
    assert ok(m=4) == L.LLFE_ERR_INVALID and ok(m=-1) == L.LLFE_ERR_INVALID
    for field, value in (("data", 0), ("height", 0), ("width", -1), ("row_stride", 26), ("row_stride", -27)):
        bad = descs.copy()
        bad[field][1] = value
        assert ok(d=bad) == L.LLFE_ERR_INVALID, (field, value)
    wide = descs.copy()
    wide["row_stride"][1] = 27  # exactly 3 * w, and 0 (packed), are fine
    assert ok(d=wide) == L.LLFE_OK
    # 1 x 2001 under auto: the rule gives 0 x 2000
    mode, h, w = PC.ZERO_SIDE
    assert PC.rule(h, w, mode)[:2] == (0, 2000)
    zero = descs.copy()
    zero["height"][1], zero["width"][1], zero["row_stride"][1] = h, w, 0
    assert ok(d=zero, m=PRE[mode]) == L.LLFE_ERR_INVALID
    assert ok(d=zero, m=PRE["none"]) == L.LLFE_OK
    with pytest.raises(ValueError):
        B.preprocess_images_layout([img], "sharpest")


def test_calls_without_a_context_are_invalid():
    img = np.zeros((8, 9, 3), np.uint8)
    descs, keep, _, _, _ = B._image_descs([img], 0)
    outs = (L.LlfeResizeOut * 1)()
    s3 = np.array([4, 5, 3], np.int32)
    lib = L.lib()
    assert lib.llfe_preprocess_images(None, descs.ctypes.data, 1, 1, None, 0, outs, None) == L.LLFE_ERR_INVALID
    assert lib.llfe_resize_cv_images(None, descs.ctypes.data, 1, s3.ctypes.data, None, 0, outs, None) == L.LLFE_ERR_INVALID


def test_abi_version_and_record_size():
    assert L.lib().llfe_abi_version() == 3
    assert C.sizeof(L.LlfeResizeOut) == 24
    assert C.sizeof(L.LlfeImageResult) == 328


def test_tiling_query_and_the_seam_sizes():
    tw, th, lds_rows = B.resize_cv_images_tiling()
    assert tw > 0 and th > 0 and lds_rows > 0
    z = C.c_int32(0)
    assert L.lib().llfe_resize_cv_images_tiling(None, C.byref(z), C.byref(z)) == L.LLFE_ERR_INVALID
    cases = PC.seam_cases(tw, th)
    kinds = set()
    for c in cases[:PC.N_SEAM]:
        assert c.ow // tw >= 3 and c.ow % tw != 0 and c.oh // th >= 3 and c.oh % th != 0, c.id
        assert c.h <= 700 and c.w <= 900, c.id
    for c in cases:
        p = RC.cv_plan(c.h, c.w, 3, c.oh, c.ow, c.interp)
        assert p.kind == c.kind, c.id
        kinds.add((p.kind, p.ks if p.kind == "GENERIC" else 0))
    assert kinds == {("AREA", 0), ("AREA_FAST", 0), ("GENERIC", 2), ("GENERIC", 8)}
    by = {c.name: RC.cv_plan(c.h, c.w, 3, c.oh, c.ow, c.interp) for c in cases if c.interp == "area"}
    assert by["s2.016"].fx == pytest.approx(2.016, rel=2e-3) and (by["s2"].fx, by["s2"].fy) == (2, 2)
    assert (by["s3"].fx, by["s3"].fy) == (3, 3)
    # a scale of 31 in y: even one output row needs 31 source rows and more; more than two never fit
    assert (by["fy31"].fx, by["fy31"].fy) == (1, 31) and by["sy31.1"].fy > 31 and 2 * 31 > lds_rows > 33
    # a scale of 31.1 in x: a tile's slice of the x table has more than 31 pairs per output pixel
    assert by["sx31.1"].fx > 31 and by["fx100"].fx == 100


def _np_cases():
    tw, th, _ = B.resize_cv_images_tiling()
    out = [(c.id, c.h, c.w, c.oh, c.ow, c.interp, k) for m in PC.MODES for k, c in enumerate(PC.rule_cases(m)) if c.resized]
    out += [(c.id, c.h, c.w, c.oh, c.ow, c.interp, k) for k, c in enumerate(PC.seam_cases(tw, th))]
    return out


@pytest.mark.parametrize("case", _np_cases(), ids=lambda v: v[0])
def test_numpy_statement_agrees_with_the_oracle(case):
    """A second statement of cv2.resize (resize_cases.np_cv_resize) on every case of the tables
    (not LARGE_SIZES, which only the device test runs)."""
    _, h, w, oh, ow, interp, k = case
    got = RC.np_cv_resize(np.asarray(PC.image(h, w, k)), ow, oh, interp)
    exp = PC.expected(h, w, oh, ow, interp, k)
    assert got.shape == exp.shape and np.array_equal(got, exp)
