""""fonts" as a feature of the batched pipeline: the parts that need no GPU -- the header and
the library's exports, the feature mask, llfe_font_records' argument check, the assembly of
records with and without a font record, and the integration rules for a batcher that was
made with the feature."""
import asyncio
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd.backend import FEATURE_BITS, ImageFeatures, feature_mask, font_bits_tiling
from low_level_feature_extraction_amd.integration import analyze_features, feature_results
from low_level_feature_extraction_amd.models import FontFeatures
from low_level_feature_extraction_amd.pipeline import assemble_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("llfe_font_bits", "llfe_font_bits_tiling", "llfe_font_records")


def test_header_defines_the_feature_bit():
    text = open(os.path.join(ROOT, "include", "llfe.h")).read()
    m = re.search(r"^#define\s+LLFE_FEATURE_FONTS\s+(\d+)u?\s*$", text, re.M)
    assert m and int(m.group(1)) == 8
    assert re.search(r"^#define\s+LLFE_LAST_CALL\s+\(-1\)\s*$", text, re.M)
    for name in NEW:
        assert re.search(r"\bint\s+%s\(" % name, text), name


def test_library_exports_the_new_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in exported and name in L.SIGNATURES and hasattr(L.lib(), name), name


def test_feature_mask_knows_fonts():
    assert L.FEATURE_FONTS == 8 and FEATURE_BITS["fonts"] == 8
    assert feature_mask(("fonts",)) == 8
    assert feature_mask(("colors", "shapes", "shadows", "fonts")) == 15
    with pytest.raises(ValueError):
        feature_mask(("text",))


def test_font_records_rejects_a_null_context():
    res = (L.LlfeFontResult * 1)()
    assert L.lib().llfe_font_records(None, C.c_int64(L.LAST_CALL), res, 1) == L.LLFE_ERR_INVALID
    assert L.lib().llfe_font_records(None, C.c_int64(0), res, 1) == L.LLFE_ERR_INVALID


def test_tiling_is_whole_words_and_covers_the_image():
    for h, w in ((1, 1), (5, 7), (433, 513), (1080, 1920), (2160, 3840)):
        strip, seg = font_bits_tiling(h, w)
        assert strip > 0 and strip % 64 == 0  # a wave owns whole output words
        assert 1 <= seg <= h
    sw, sh = C.c_int32(0), C.c_int32(0)
    assert L.lib().llfe_font_bits_tiling(0, 5, C.byref(sw), C.byref(sh)) == L.LLFE_ERR_INVALID
    assert L.lib().llfe_font_bits_tiling(5, 5, None, C.byref(sh)) == L.LLFE_ERR_INVALID


def _record(font):
    r = ImageFeatures(np.zeros((0, 3), np.uint8), np.zeros(0, np.int64), 0, 0.0, 10, 2, width=40, height=30)
    r.font = font
    return r


def test_image_features_font_defaults_to_none():
    r = ImageFeatures(np.zeros((0, 3), np.uint8), np.zeros(0, np.int64), 0, 0.0, 0, 0)
    assert r.font is None


def test_assemble_batch_with_and_without_font_records():
    hit = {"n_contours": 3, "n_regions": 2, "x": 4, "y": 5, "width": 30, "height": 20, "gray_sum": 30 * 20 * 200}
    miss = {"n_contours": 1, "n_regions": 0, "x": 0, "y": 0, "width": 0, "height": 0, "gray_sum": 0}
    out = assemble_batch([_record(hit), _record(miss)], ("shadows", "fonts"))
    assert [set(o) for o in out] == [{"shadows", "fonts"}] * 2
    f = out[0]["fonts"]
    assert isinstance(f, FontFeatures)
    assert (f.font_family, f.font_size, f.font_style, f.confidence) == ("Arial", 15.0, "Regular", 0.8)
    assert out[1]["fonts"] is None  # no region: what detect_font returns
    # stub records of an older shape (no .font) still assemble the other features
    stub = SimpleNamespace(shadow_sum=0, shadow_count=0, shadow_level="Low")
    assert assemble_batch([stub], ("shadows",)) == [{"shadows": {"shadow_level": "Low"}}]
    # ... and asking for fonts of a record that has none is an error, not a silent None
    with pytest.raises(ValueError):
        assemble_batch([stub], ("fonts",))
    with pytest.raises(ValueError):
        assemble_batch([_record(None)], ("fonts",))


FONT = FontFeatures(font_family="Arial", font_size=12.0, font_style="Bold", confidence=0.8)
BATCHED = {"colors": "C", "shapes": "S", "shadows": "D"}


def test_feature_results_takes_fonts_from_the_batch_when_it_holds_them():
    order = ["text", "fonts", "colors"]
    out = feature_results(order, dict(BATCHED, fonts=FONT), {"text": lambda: "T", "fonts": lambda: "extra"})
    assert out == ["T", FONT, "C"]
    # a batch without fonts: exactly as before -- extra, else the "not computed" error
    out = feature_results(order, BATCHED, {"text": lambda: "T", "fonts": lambda: "extra"})
    assert out == ["T", "extra", "C"]
    out = feature_results(order, BATCHED, {"text": lambda: "T"})
    assert isinstance(out[1], ValueError) and "fonts" in str(out[1]) and out[2] == "C"
    # a batch that found no region holds fonts = None, and that is the result
    assert feature_results(["fonts"], dict(BATCHED, fonts=None), {"fonts": lambda: "extra"}) == [None]
    # a failed batch does not swallow an extra fonts extractor
    boom = RuntimeError("gpu batch failed")
    out = feature_results(order, boom, {"text": lambda: "T", "fonts": lambda: "extra"})
    assert out == ["T", "extra", boom]


class _Batcher:
    def __init__(self, features, result):
        self.features, self.result, self.calls = tuple(features), result, 0

    async def analyze(self, image):
        self.calls += 1
        if isinstance(self.result, BaseException):
            raise self.result
        return dict(self.result)


def test_analyze_features_calls_a_batcher_bound_with_fonts():
    img = np.zeros((4, 4, 3), np.uint8)
    mb = _Batcher(("colors", "fonts"), {"colors": "C", "fonts": FONT})
    assert asyncio.run(analyze_features(img, ["fonts"], mb)) == [FONT] and mb.calls == 1
    assert asyncio.run(analyze_features(img, ["text", "fonts", "colors"], mb, {"text": lambda: "T"})) == ["T", FONT, "C"]
    # a default batcher is not called for fonts alone, and fonts stays with extra / the error
    mb = _Batcher(("colors", "shapes", "shadows"), BATCHED)
    out = asyncio.run(analyze_features(img, ["fonts"], mb))
    assert mb.calls == 0 and isinstance(out[0], ValueError)
    assert asyncio.run(analyze_features(img, ["fonts"], mb, {"fonts": lambda: "extra"})) == ["extra"] and mb.calls == 0
    # a stand-in without a features attribute behaves as before
    class Bare:
        async def analyze(self, image):
            return dict(BATCHED)

    assert asyncio.run(analyze_features(img, ["fonts", "shapes"], Bare(), {"fonts": lambda: "extra"})) == ["extra", "S"]
    # the batch fails: the error stays on the hot-path features, extra fonts still answers
    boom = RuntimeError("gpu batch failed")
    out = asyncio.run(analyze_features(img, ["colors", "fonts"], _Batcher(("colors", "fonts"), boom),
                                       {"fonts": lambda: "extra"}))
    assert out == [boom, "extra"]
