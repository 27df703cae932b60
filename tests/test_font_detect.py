"""llfe_font_detect (font.hip + the boxes-only contour pass): FontDetector.detect_font's
regions, largest region and gray sum on the device.

Expected values always come from the oracle: adaptive_threshold_inv(bgr2gray(img)),
find_contours_external, bounding_rect, then the reference's rules in Python (reference
app/services/analyze/font_detector.py:39-67, 109-155).  Every field of the record is
compared and, where asked for, the whole region list."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import synth
from low_level_feature_extraction_amd.font_detector import FontDetector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("n_contours", "n_regions", "x", "y", "width", "height", "gray_sum")


# ------------------------------------------------------------------ the oracle's restatement
def _oracle_record(orc, binary, img=None):
    """The record llfe_font_detect must return for one binary (and its BGR image)."""
    contours = orc.find_contours_external(np.ascontiguousarray(binary))
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
        if img is not None:
            g = orc.bgr2gray(np.ascontiguousarray(img[y:y + h, x:x + w]))
            rec["gray_sum"] = int(g.sum(dtype=np.uint64))
    return rec


def _oracle_image_record(orc, img):
    return _oracle_record(orc, orc.adaptive_threshold_inv(orc.bgr2gray(img)), img)


def _oracle_features(orc, img):
    binary = orc.adaptive_threshold_inv(orc.bgr2gray(img))
    rec = _oracle_record(orc, binary, img)
    if not rec["n_regions"]:
        return None
    x, y, w, h = rec["x"], rec["y"], rec["width"], rec["height"]
    m = np.mean(orc.bgr2gray(np.ascontiguousarray(img[y:y + h, x:x + w])))
    weight = "Light" if m >= 250 else ("Regular" if m > 190 else "Bold")
    return ("Arial", float(int(h * 0.75)), weight, 0.8)


def _features(f):
    return None if f is None else (f.font_family, f.font_size, f.font_style, f.confidence)


def _same(got, exp, what=""):
    for f in FIELDS:
        assert got[f] == exp[f], (what, f, got[f], exp[f])
    if "regions" in got:
        assert got["regions"] == exp["regions"], what


def _check_binaries(backend, orc, binaries, images=None):
    """font_detect over crafted binaries (no gray sums without images) -> the records"""
    binaries = np.ascontiguousarray(binaries, np.uint8)
    got = backend.font_detect(images, binary=binaries, regions=True)
    assert len(got) == len(binaries)
    for i, b in enumerate(binaries):
        _same(got[i], _oracle_record(orc, (b != 0).astype(np.uint8) * 255, None if images is None else images[i]), i)
    return got


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


# ------------------------------------------------------------------ CPU
def test_library_exports_llfe_font_detect():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "llfe_font_detect" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert "llfe_font_detect" in L.SIGNATURES and hasattr(L.lib(), "llfe_font_detect")


def test_font_result_layout_matches_header(tmp_path):
    assert C.sizeof(L.LlfeFontResult) == 40
    fields = [f for f, _ in L.LlfeFontResult._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "llfe.h"', "int main(void){",
             'printf("sizeof %zu\\n", sizeof(llfe_font_result));']
    lines += [f'printf("{f} %zu\\n", offsetof(llfe_font_result, {f}));' for f in fields]
    lines.append("return 0;}")
    src, exe = tmp_path / "lay.c", tmp_path / "lay"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                   check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(L.LlfeFontResult)
    for f in fields:
        assert int(got[f]) == getattr(L.LlfeFontResult, f).offset, f


def test_null_context_is_invalid():
    res = (L.LlfeFontResult * 1)()
    need = C.c_int64(0)
    assert L.lib().llfe_font_detect(None, None, None, 1, 4, 4, res, None, 0, C.byref(need), None) == L.LLFE_ERR_INVALID


# ------------------------------------------------------------------ GPU: crafted binaries
@pytest.mark.gpu
def test_filter_boundaries(backend, orc):
    b = np.zeros((60, 200), np.uint8)
    b[2:11, 3:4] = 255       # 1 x 9 column: 0.111 -> kept
    b[2:12, 8:9] = 255       # 1 x 10 column: aspect exactly 0.1 -> dropped
    b[14:22, 3:23] = 255     # 20 x 8 block: h == 8 -> dropped
    b[26:35, 3:138] = 255    # 135 x 9 bar: aspect exactly 15 -> dropped
    b[40:49, 3:137] = 255    # 134 x 9 bar: kept
    got = _check_binaries(backend, orc, b[None])[0]
    assert got["n_contours"] == 5 and sorted(got["regions"]) == [(3, 2, 1, 9), (3, 40, 134, 9)]


@pytest.mark.gpu
def test_ties_go_to_the_first_in_list_order(backend, orc):
    b = np.zeros((80, 120), np.uint8)
    b[5:15, 5:25] = 255      # 20 x 10
    b[30:50, 40:50] = 255    # 10 x 20
    b[60:70, 80:100] = 255   # 20 x 10
    b[20:29, 100:104] = 255  # smaller ones
    b[52:62, 10:19] = 255
    got = _check_binaries(backend, orc, np.stack([b, b[::-1].copy(), b[:, ::-1].copy()]))
    exp = _oracle_record(orc, b)
    first_max = next(r for r in exp["regions"] if r[2] * r[3] == 200)
    assert (got[0]["x"], got[0]["y"], got[0]["width"], got[0]["height"]) == first_max
    assert sum(r[2] * r[3] == 200 for r in got[0]["regions"]) == 3


@pytest.mark.gpu
def test_nesting_counts_external_contours_only(backend, orc):
    from scipy import ndimage

    b = np.zeros((90, 130), np.uint8)
    b[10:60, 10:70] = 255    # a thick ring ...
    b[20:50, 20:60] = 0
    b[28:42, 30:50] = 255    # ... with a blob inside its hole
    b[0:40, 85:130] = 255    # a hole that touches the image border ...
    b[0:30, 95:130] = 0
    b[5:20, 105:120] = 255   # ... with a blob inside
    b[70:85, 20:40] = 255    # and a plain block
    ncomp = ndimage.label(b, structure=np.ones((3, 3)))[1]
    got = _check_binaries(backend, orc, b[None])[0]
    assert got["n_contours"] < ncomp  # not "every component is a contour"


@pytest.mark.gpu
@pytest.mark.parametrize("b", [np.zeros((40, 50), np.uint8), np.full((12, 12), 255, np.uint8),
                               np.zeros((1, 1), np.uint8), np.full((1, 1), 255, np.uint8)],
                         ids=["zeros", "full12", "one0", "one255"])
def test_degenerate_masks(backend, orc, b):
    got = _check_binaries(backend, orc, b[None])[0]
    if b.shape == (12, 12):
        assert got["n_regions"] == 1 and got["regions"] == [(0, 0, 12, 12)]
    else:
        assert got["n_regions"] == 0 and (got["x"], got["y"], got["width"], got["height"], got["gray_sum"]) == (0,) * 5


@pytest.mark.gpu
def test_nonzero_is_foreground_and_gray_sum_of_the_winner(backend, orc):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 50, 70, 3), dtype=np.uint8)
    b = np.zeros((2, 50, 70), np.uint8)
    b[0, 4:30, 6:40] = 1
    b[0, 35:47, 3:60] = 200
    b[1, 10:20, 10:15] = 255
    got = _check_binaries(backend, orc, b, img)
    assert got[0]["gray_sum"] > 0 and got[1]["gray_sum"] > 0


def _sparse(h, w, seed, p):
    rng = np.random.default_rng(seed)
    b = (rng.random((h, w)) < p).astype(np.uint8) * 255
    b[2:14, 5:40] = 255
    b[h - 12:h - 1, w - 30:w - 2] = 255
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(40, 257), (24, 4033)])
def test_bit_row_geometry(backend, orc, h, w):
    got = _check_binaries(backend, orc, _sparse(h, w, 11, 0.03)[None])[0]
    assert got["n_regions"] >= 2


@pytest.mark.gpu
def test_too_wide_comes_back_through_the_host_path(backend, orc):
    b = _sparse(12, 4100, 12, 0.03)
    with pytest.raises(L.LlfeError) as e:
        backend.font_detect(None, binary=b[None], regions=True)
    assert e.value.code == L.LLFE_ERR_UNSUPPORTED
    exp = _oracle_record(orc, b)
    assert FontDetector.detect_text_regions_batch(b[None]) == [exp["regions"]] and exp["n_regions"] >= 1
    img = np.random.default_rng(1).integers(0, 256, (12, 4100, 3), dtype=np.uint8)
    assert _features(FontDetector.detect_font_batch(img[None])[0]) == _oracle_features(orc, img)


@pytest.mark.gpu
def test_component_capacity_regrowth(orc):
    """7 746 8-connected components in the random part, above the default capacity of
    n * 1024 + 4096 = 5 120 for one image: the pass grows its capacities and reruns."""
    from low_level_feature_extraction_amd.backend import Backend

    b = (np.random.default_rng(5).random((300, 400)) < 0.1).astype(np.uint8) * 255
    b[100:112, 50:80] = 255  # 30 x 12: a region exists
    exp = _oracle_record(orc, b)
    assert exp["n_contours"] > 5120 and exp["n_regions"] > 0
    be = Backend(0)
    try:
        _same(be.font_detect(None, binary=b[None], regions=True)[0], exp)
        _same(be.font_detect(None, binary=b[None])[0], exp)  # grown capacities kept
    finally:
        be.close()


@pytest.mark.gpu
def test_region_list_protocol(backend, orc):
    import torch

    rng = np.random.default_rng(9)
    b = np.zeros((5, 64, 96), np.uint8)
    for i in (0, 1, 3, 4):  # image 2 stays empty
        for _ in range(2 + i):
            y, x = int(rng.integers(0, 50)), int(rng.integers(0, 70))
            b[i, y:y + int(rng.integers(9, 14)), x:x + int(rng.integers(4, 26))] = 255
    exp = [_oracle_record(orc, m) for m in b]
    total = sum(e["n_regions"] for e in exp)
    assert total >= 5 and exp[2]["n_regions"] == 0
    d = torch.from_numpy(b).to("cuda:0")
    lib = L.lib()

    def call(cap, with_list=True):
        res = (L.LlfeFontResult * 5)()
        reg = np.full((max(cap, 1), 4), -1, np.int32)
        need = C.c_int64(-1)
        rc = lib.llfe_font_detect(backend.ctx, None, d.data_ptr(), 5, 64, 96, res, reg.ctypes.data if with_list else None,
                                  cap, C.byref(need), None)
        return rc, res, reg, need.value

    def records_ok(res):
        off = 0
        for i in range(5):
            for f in FIELDS:
                assert getattr(res[i], f) == exp[i][f], (i, f)
            assert res[i].region_offset == off
            off += exp[i]["n_regions"]

    rc, res, reg, need = call(total - 1)
    assert rc == L.LLFE_ERR_CAPACITY and need == total
    records_ok(res)  # results stay valid
    assert reg[:total - 1].tolist() == [list(r) for e in exp for r in e["regions"]][:total - 1]
    rc, res, reg, need = call(total)
    assert rc == L.LLFE_OK and need == total
    records_ok(res)
    for i in range(5):
        o = res[i].region_offset
        assert [tuple(v) for v in reg[o:o + res[i].n_regions].tolist()] == exp[i]["regions"]
    rc, res, reg, need = call(0, with_list=False)  # summary only
    assert rc == L.LLFE_OK and need == total
    records_ok(res)
    assert lib.llfe_font_detect(backend.ctx, None, None, 5, 64, 96, res, None, 0, None, None) == L.LLFE_ERR_INVALID


@pytest.mark.gpu
def test_chunked_batch_keeps_global_region_offsets(backend, orc, monkeypatch):
    """A workspace budget of one image per device pass: five passes, one answer."""
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (5, 48, 80, 3), dtype=np.uint8)
    b = np.zeros((5, 48, 80), np.uint8)
    for i in (0, 1, 2, 4):  # image 3 stays empty
        for _ in range(1 + i):
            y, x = int(rng.integers(0, 34)), int(rng.integers(0, 54))
            b[i, y:y + int(rng.integers(9, 14)), x:x + int(rng.integers(4, 26))] = 255
    whole = _check_binaries(backend, orc, b, img)
    monkeypatch.setenv("LLFE_WORKSPACE_GB", "0.001")
    assert backend.batch_capacity(48, 80) == 1
    chunked = _check_binaries(backend, orc, b, img)
    assert chunked == whole and sum(r["n_regions"] for r in whole) >= 4


@pytest.mark.gpu
def test_refused_while_a_submitted_batch_is_uncollected(backend, orc):
    imgs = np.stack([_glyphs(64, 128, s) for s in range(2)])
    t = backend.submit(imgs, ("shadows",), seed=1)
    try:
        with pytest.raises(L.LlfeError) as e:
            backend.font_detect(imgs)
        assert e.value.code == L.LLFE_ERR_INVALID
    finally:
        backend.collect(t)
    for got, im in zip(backend.font_detect(imgs, regions=True), imgs):
        _same(got, _oracle_image_record(orc, im))


@pytest.mark.gpu
@pytest.mark.parametrize("fill,dent,style", [(250, None, "Light"), (250, 249, "Regular"), (191, None, "Regular"),
                                             (190, None, "Bold"), (191, 190, "Regular")])
def test_exact_mean_at_the_weight_thresholds(backend, orc, fill, dent, style):
    img = np.full((40, 44, 3), fill, np.uint8)
    if dent is not None:
        img[17, 13] = dent
    b = np.zeros((40, 44), np.uint8)
    b[8:28, 10:20] = 255  # 10 x 20
    got = _check_binaries(backend, orc, b[None], img[None])[0]
    assert (got["width"], got["height"]) == (10, 20)
    assert got["gray_sum"] == int(orc.bgr2gray(np.ascontiguousarray(img[8:28, 10:20])).sum())
    f = FontDetector._from_record(got)
    m = np.mean(orc.bgr2gray(np.ascontiguousarray(img[8:28, 10:20])))
    assert f.font_style == style == ("Light" if m >= 250 else ("Regular" if m > 190 else "Bold"))
    assert (f.font_family, f.font_size, f.confidence) == ("Arial", 15.0, 0.8)


# ------------------------------------------------------------------ GPU: from BGR
def _bgr_cases():
    rng = np.random.default_rng(77)
    cases = [(f"random{h}x{w}", rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8))
             for h, w in [(1, 1), (5, 7), (3, 257), (31, 33), (100, 37), (150, 404)]]
    cases.append(("glyphs", np.stack([_glyphs(240, 320, s) for s in range(3)] + [np.full((240, 320, 3), 128, np.uint8)])))
    cases.append(("synth", np.stack([synth.synth_numpy(0, 270, 480, seed=5, kind="ui"),
                                     synth.synth_numpy(1, 270, 480, seed=5, kind="photo")])))
    return cases


@pytest.fixture(scope="module")
def bgr_runs(backend, orc):
    """(name, images, device records with lists, oracle records) of every BGR case, once"""
    runs = []
    for name, imgs in _bgr_cases():
        runs.append((name, imgs, backend.font_detect(imgs, regions=True), [_oracle_image_record(orc, im) for im in imgs]))
    return runs


@pytest.mark.gpu
def test_from_bgr_vs_oracle(bgr_runs):
    seen = set()
    for name, imgs, got, exp in bgr_runs:
        for i in range(len(imgs)):
            _same(got[i], exp[i], (name, i))
            seen.add(exp[i]["n_regions"] > 0)
    assert seen == {True, False}  # both branches ran


@pytest.mark.gpu
def test_batch_record_equals_single_image_record(backend, bgr_runs):
    for name, imgs, got, _ in bgr_runs:
        for i in range(len(imgs)):
            _same(backend.font_detect(imgs[i:i + 1], regions=True)[0], got[i], (name, i))


@pytest.mark.gpu
def test_numpy_and_device_tensor_give_equal_features(orc, bgr_runs):
    import torch

    for name, imgs, _, _ in bgr_runs[-2:]:
        a = FontDetector.detect_font_batch(imgs)
        t = FontDetector.detect_font_batch(torch.from_numpy(imgs).to("cuda:0"))
        assert [_features(f) for f in a] == [_features(f) for f in t] == [_oracle_features(orc, im) for im in imgs], name
        assert _features(FontDetector.detect_font(imgs[0])) == _features(a[0])


@pytest.mark.gpu
def test_detect_text_regions_batch_on_the_device(backend, orc, bgr_runs):
    name, imgs, _, exp = bgr_runs[-2]
    binaries = backend.font_binary(imgs)  # a device tensor: stays there
    assert FontDetector.detect_text_regions_batch(binaries) == [e["regions"] for e in exp]
    assert FontDetector.detect_text_regions(binaries[0].cpu().numpy()) == exp[0]["regions"]


@pytest.mark.gpu
def test_kernels_are_reported_by_kernel_stats(backend):
    backend.set_profiling(True)
    try:
        backend.font_detect(_glyphs(240, 320, 1)[None], regions=True)
        stats = backend.kernel_stats()
    finally:
        backend.set_profiling(False)
    for k in ("k_font_binary", "k_font_pack", "k_contours_boxes", "k_font_select", "k_font_gray_sum", "k_font_regions"):
        assert stats[k]["launches"] >= 1, k
