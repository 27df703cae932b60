"""The host side of the one-pass shapes and shadows of a mixed-size batch
(llfe_shapes_images_layout, the flag checks of llfe_process_images_routes, the ``shapes=``
option) and the compiled shape of the ragged k_ccl_runs: no GPU.  Every expected value is derived
here from the image sizes, not read back from the planner."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import backend as B

# the size ladder of tests/test_gpu_shapes_images.py: (height, width)
LADDER = [(1, 1), (2, 3), (5, 7), (11, 12), (64, 240), (65, 241), (40, 256), (40, 257), (216, 8), (217, 9), (433, 16),
          (30, 479), (30, 480), (30, 481), (63, 65), (130, 200), (3, 488), (13, 728), (229, 488)]
STRIP, SEG, TILE = 240, 216, 64
MAX_TILES = 2**31 // 4096  # 524288: the ids tile * 4096 + node are int
TILE_BYTES = 4096 * 7 + 512 + 20  # llfe.h, llfe_shapes_images_layout


def _images(sizes):
    return [np.zeros((h, w, 3), np.uint8) for h, w in sizes]


def _ceil(a, b):
    return -(-a // b)


def _geometry(h, w):
    """stream_geometry(h, w): strips of 240 columns, about-216-row segments of equal length."""
    segs = max(1, _ceil(h, SEG))
    seg_rows = _ceil(h, segs)
    return _ceil(w, STRIP), _ceil(h, seg_rows), seg_rows


def _workspace(p):
    return 3 * p["class_bytes"] + TILE_BYTES * p["tiles"] + 16 * p["words"] + p["stage_bytes"] + 8 * p["work_count"]


@pytest.mark.parametrize("sizes", [LADDER, LADDER[::-1]], ids=["input", "reversed"])
def test_layout_of_the_size_ladder(sizes):
    recs, work, passes = B.shapes_images_layout(_images(sizes))
    assert len(recs) == len(sizes) and len(passes) == 1
    tile = word = part = 0
    end = 0
    expect_work = []
    for i, ((h, w), r) in enumerate(zip(sizes, recs)):
        strips, segs, seg_rows = _geometry(h, w)
        assert (r["height"], r["width"], r["pixels"]) == (h, w, h * w)
        assert (r["strips"], r["segs"], r["seg_rows"]) == (strips, segs, seg_rows), (h, w)
        assert (r["tiles_x"], r["tiles_y"]) == (_ceil(w, TILE), _ceil(h, TILE))
        assert r["pass"] == 0 and r["resized"] == 0
        # tile, word and partial offsets are the prefix sums
        assert (r["first_tile"], r["word_offset"], r["first_part"]) == (tile, word, part), (i, h, w)
        tile += _ceil(w, TILE) * _ceil(h, TILE)
        word += h * _ceil(w, 64)
        part += strips * segs
        # class maps: 16-byte aligned, one behind the other without overlap
        assert r["class_offset"] % 16 == 0 and end <= r["class_offset"] < end + 16
        end = r["class_offset"] + h * w
        # host arrays: every one is staged, packed, at an aligned offset
        assert r["stage_offset"] % 16 == 0
        expect_work += [(i, st, sg) for sg in range(segs) for st in range(strips)]
    # every (image, strip, segment) exactly once, in image order
    assert [(e["image"], e["strip"], e["seg"]) for e in work] == expect_work
    assert len(set(expect_work)) == len(expect_work) == part
    p = passes[0]
    assert (p["first"], p["count"], p["work_first"], p["work_count"]) == (0, len(sizes), 0, part)
    assert (p["tiles"], p["words"], p["first_word"]) == (tile, word, 0)
    assert end <= p["class_bytes"] < end + 16 and p["class_bytes"] % 16 == 0
    assert p["workspace_bytes"] == _workspace(p)


def test_the_ladder_has_fast_waves():
    """What the GPU ladder's comment claims of its widest shapes: each has a strip whose whole
    window lies inside the image (a `fast` wave, W % 4 == 0), 13 x 728 has two, and 229 x 488 has
    two segments, so a `fast` wave's segment ends inside the image."""
    from tests import stencil_cases as SC

    for h, w in ((3, 488), (13, 728), (229, 488)):
        assert (h, w) in LADDER and w % 4 == 0
        assert SC.fast_strips(w), (h, w)
        assert SC.geometry(h, w) == _geometry(h, w)
    assert SC.fast_strips(488) == [1] and SC.fast_strips(728) == [1, 2]
    assert SC.geometry(3, 488)[1] == SC.geometry(13, 728)[1] == 1
    assert SC.geometry(229, 488)[1:] == (2, 115)
    assert not any(SC.fast_strips(w) for h, w in LADDER if w < 488)  # (no other shape of the ladder has one)


def test_every_image_has_at_least_as_many_tiles_as_waves():
    for h in (1, 63, 64, 65, 215, 216, 217, 432, 433, 1080, 5000):
        for w in (1, 64, 239, 240, 241, 1920, 7000):
            strips, segs, _ = _geometry(h, w)
            assert strips * segs <= _ceil(w, TILE) * _ceil(h, TILE), (h, w)


def test_pass_cutting_under_a_budget(monkeypatch):
    monkeypatch.setenv("LLFE_WORKSPACE_GB", "0.002")  # 2 MB: the ladder's 130 tiles alone need 3.8 MB
    budget = 0.002e9
    sizes = LADDER + [(130, 200), (64, 64), (300, 300)]
    recs, work, passes = B.shapes_images_layout(_images(sizes))
    assert len(passes) >= 2
    nxt = nwork = nword = 0
    for k, p in enumerate(passes):  # consecutive, in input order, every image once
        assert p["first"] == nxt and p["count"] >= 1
        assert (p["work_first"], p["first_word"]) == (nwork, nword)
        members = recs[p["first"]:p["first"] + p["count"]]
        assert all(r["pass"] == k for r in members)
        assert p["tiles"] == sum(r["tiles_x"] * r["tiles_y"] for r in members) < MAX_TILES
        assert p["words"] == sum(r["height"] * _ceil(r["width"], 64) for r in members)
        assert p["workspace_bytes"] == _workspace(p)
        assert p["workspace_bytes"] <= budget or p["count"] == 1  # (one image always makes a pass)
        assert members[0]["first_tile"] == members[0]["word_offset"] == members[0]["class_offset"] == 0
        nxt += p["count"]
        nwork += p["work_count"]
        nword += p["words"]
    assert nxt == len(sizes) and nwork == len(work)
    # greedy: the next pass's first image would not have fitted
    for p, q in zip(passes, passes[1:]):
        r = recs[q["first"]]
        grown = dict(p, tiles=p["tiles"] + r["tiles_x"] * r["tiles_y"], words=p["words"] + r["height"] * _ceil(r["width"], 64),
                     class_bytes=(p["class_bytes"] + r["pixels"] + 15) // 16 * 16,
                     stage_bytes=(p["stage_bytes"] + 3 * r["pixels"] + 15) // 16 * 16,
                     work_count=p["work_count"] + r["strips"] * r["segs"])
        assert _workspace(grown) > budget


def test_no_pass_reaches_the_tile_limit():
    one = np.zeros((1, 1, 3), np.uint8)  # one tile each
    n = MAX_TILES + 10
    lib = L.lib()
    descs = np.zeros(n, np.dtype(L.LlfeImageDesc))
    descs["data"], descs["height"], descs["width"] = one.ctypes.data, 1, 1
    nw, npass = C.c_int64(0), C.c_int32(0)
    passes = (L.LlfeShapePass * 4)()
    assert lib.llfe_shapes_images_layout(descs.ctypes.data, n, 0, None, None, 0, C.byref(nw), passes, 4,
                                         C.byref(npass)) == L.LLFE_OK
    assert nw.value == n and npass.value == 2
    assert [passes[k].count for k in range(2)] == [MAX_TILES - 1, 11]
    assert all(passes[k].tiles < MAX_TILES for k in range(2))


def test_invalid_descriptors_are_refused():
    lib = L.lib()
    d = np.zeros(2, np.dtype(L.LlfeImageDesc))
    buf = np.zeros(64 * 3, np.uint8)
    d["data"], d["height"], d["width"] = buf.ctypes.data, 4, 4
    nw, npass = C.c_int64(0), C.c_int32(0)

    def plan(descs=d, n=2, mode=0):
        return lib.llfe_shapes_images_layout(descs.ctypes.data if descs is not None else None, n, mode, None, None, 0,
                                             C.byref(nw), None, 0, C.byref(npass))

    assert plan() == L.LLFE_OK and (nw.value, npass.value) == (2, 1)
    assert plan(n=0) == L.LLFE_OK and (nw.value, npass.value) == (0, 0)
    assert plan(n=-1) == L.LLFE_ERR_INVALID
    assert plan(descs=None) == L.LLFE_ERR_INVALID
    assert plan(mode=7) == L.LLFE_ERR_INVALID
    for field, value in (("data", 0), ("height", 0), ("width", -3), ("row_stride", 11)):
        bad = d.copy()
        bad[field][1] = value
        assert plan(descs=bad) == L.LLFE_ERR_INVALID, field
    # a work table or a pass list that is too short: the counts are still filled
    work = (L.LlfeShapeWork * 1)()
    nw.value = npass.value = 0
    assert lib.llfe_shapes_images_layout(d.ctypes.data, 2, 0, None, work, 1, C.byref(nw), None, 0,
                                         C.byref(npass)) == L.LLFE_ERR_CAPACITY
    assert (nw.value, npass.value) == (2, 1)


def test_abi_version_struct_sizes_and_flag_bits():
    lib = L.lib()
    assert lib.llfe_abi_version() == 3
    assert C.sizeof(L.LlfeShapeImage) == 80 and C.sizeof(L.LlfeShapeWork) == 12 and C.sizeof(L.LlfeShapePass) == 64

    def routes(cflags, sflags):  # (no context: flag words that pass their check go on to the NULL-context refusal)
        return lib.llfe_process_images_routes(None, None, 0, 0, 0, 5, 0, 0, None, None, 0, None, None, cflags, sflags)

    for ok in ((0, 0), (1, 0), (0, L.IMAGES_SHAPES_ONE_PASS), (L.IMAGES_COLORS_ONE_PASS, L.IMAGES_SHAPES_ONE_PASS)):
        assert routes(*ok) == L.LLFE_ERR_INVALID, ok
    for unknown in (2, 4, 1 << 31, 3):
        assert routes(unknown, 0) == L.LLFE_ERR_UNSUPPORTED, unknown
        assert routes(0, unknown) == L.LLFE_ERR_UNSUPPORTED, unknown
        assert routes(1, unknown) == L.LLFE_ERR_UNSUPPORTED, unknown

    def flags(word):  # the existing entry keeps its own check
        return lib.llfe_process_images_flags(None, None, 0, 0, 0, 5, 0, 0, None, None, 0, None, None, word)

    assert flags(0) == L.LLFE_ERR_INVALID and flags(1) == L.LLFE_ERR_INVALID
    for unknown in (2, 3, 4):
        assert flags(unknown) == L.LLFE_ERR_UNSUPPORTED, unknown


def test_shapes_option_is_checked_without_a_gpu():
    from low_level_feature_extraction_amd.color_extractor import ColorExtractor
    from low_level_feature_extraction_amd.pipeline import run_batch
    from low_level_feature_extraction_amd.shadow_analyzer import ShadowAnalyzer
    from low_level_feature_extraction_amd.shape_analyzer import ShapeAnalyzer

    assert B.shapes_flags("grouped") == 0 and B.shapes_flags("one_pass") == L.IMAGES_SHAPES_ONE_PASS
    for bad in ("onepass", "single", "", None, 1):
        with pytest.raises(ValueError):
            B.shapes_flags(bad)
    imgs = _images([(4, 4), (5, 3)])
    with pytest.raises(ValueError):
        run_batch(imgs, ("shapes",), shapes="single")
    with pytest.raises(ValueError):
        ShapeAnalyzer.analyze_shapes_batch(imgs, shapes="single")
    with pytest.raises(ValueError):
        ShadowAnalyzer.analyze_shadow_level_batch(imgs, shapes="single")
    with pytest.raises(ValueError):
        ColorExtractor.extract_colors_batch(imgs, shapes="single")


# ------------------------------------------------------------------ compiled structure
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "low_level_feature_extraction_amd", "csrc", "hysteresis.hip")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not available")


def _tile_loop_structure(asm: str, symbol: str):
    """The checks of tests/test_ccl_isa.py on the function whose mangled name contains `symbol`."""
    m = re.search(r"^(_Z\S*" + re.escape(symbol) + r"\S*):", asm, re.M)
    assert m, f"{symbol} not in the ISA"
    lines = asm[m.start():asm.index("s_endpgm", m.start())].splitlines()
    d1 = [i for i, ln in enumerate(lines) if "Loop Header: Depth=1" in ln]
    d2 = [i for i, ln in enumerate(lines) if "Loop Header: Depth=2" in ln]
    assert len(d1) == 1, f"{symbol}: expected one outer (work-counter) loop"
    assert len(d2) == 1, f"{symbol}: expected exactly one depth-2 loop"
    head = lines[d1[0]:d2[0]]
    atom = [i for i, ln in enumerate(head) if "global_atomic_add" in ln]
    bars = [i for i, ln in enumerate(head) if re.search(r"\bs_barrier\b", ln)]
    lds = [i for i, ln in enumerate(head) if "ds_read_b32" in ln]
    assert atom and len(bars) == 2 and lds, f"{symbol}: counter atomic, two barriers and the LDS read in the outer header"
    assert atom[0] < bars[0] < lds[0] < bars[1], f"{symbol}: atomic -> barrier -> LDS base read -> barrier"
    assert not any(re.search(r"ds_bpermute|v_readlane|ds_swizzle", ln) for ln in head), symbol
    assert not any(re.search(r"\bs_barrier\b", ln) for ln in lines[d2[0]:]), f"{symbol}: a barrier inside the tile loop"


def test_ragged_k_ccl_runs_has_the_uniform_tile_loop_structure(tmp_path):
    out = tmp_path / "hyst.s"
    from low_level_feature_extraction_amd import _build
    cmd = [_hipcc(), *_build.compile_flags("hysteresis.hip"), "--cuda-device-only", "-S", SRC, "-o", str(out)]  # build()'s flags
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    asm = out.read_text()
    # k_ccl_runs<false> / <true>: the Itanium mangling of the bool template argument
    _tile_loop_structure(asm, "k_ccl_runsILb0E")
    _tile_loop_structure(asm, "k_ccl_runsILb1E")
