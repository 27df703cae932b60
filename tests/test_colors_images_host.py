"""The host side of the one-pass colours of a mixed-size batch (llfe_colors_images_layout,
the flag check of llfe_process_images_flags, the ``colors=`` option): no GPU.  Every expected
value is derived here from the pixel counts, not read back from the planner."""
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import backend as B

# the size ladder of tests/test_gpu_colors_images.py: (height, width)
LADDER = [(1, 1), (3, 5), (4, 4), (1, 17), (33, 31), (32, 32), (63, 65), (64, 64), (17, 241), (3, 2731), (150, 96),
          (90, 160)]
STEP = 4096  # pixels per scatter step
MAX_PASS = 4096  # kMaxKmeansBatch


def _images(sizes):
    return [np.zeros((h, w, 3), np.uint8) for h, w in sizes]


def _ceil(a, b):
    return -(-a // b)


def test_records_of_the_size_ladder():
    recs, work, passes = B.colors_images_layout(_images(LADDER))
    assert len(recs) == len(LADDER) and len(passes) == 1
    for (h, w), r in zip(LADDER, recs):
        P = h * w
        assert (r["height"], r["width"], r["pixels"]) == (h, w, P)
        assert r["field_pixels"] == 16 * _ceil(P, 16)
        assert r["steps"] == _ceil(P, STEP)
        assert r["pass"] == 0 and r["resized"] == 0
    pmax = max(h * w for h, w in LADDER)
    p = passes[0]
    assert (p["first"], p["count"], p["max_pixels"]) == (0, len(LADDER), pmax)
    assert p["key_stride"] == (pmax + 3) // 4 * 4
    assert p["cube_stride"] == min(p["key_stride"], 1 << 18)
    assert p["cell_stride"] == min(p["cube_stride"], 64 * 1024)
    assert p["tab_steps"] == _ceil(pmax, STEP)
    assert (p["work_first"], p["work_count"]) == (0, len(work))


def test_host_images_are_staged_at_aligned_offsets():
    recs, _, passes = B.colors_images_layout(_images(LADDER))
    end = 0
    for (h, w), r in zip(LADDER, recs):  # host arrays: every one is staged, packed, in input order
        assert r["stage_offset"] % 16 == 0 and r["stage_offset"] >= end
        end = r["stage_offset"] + 3 * h * w
    assert passes[0]["stage_bytes"] >= end and passes[0]["stage_bytes"] % 16 == 0


@pytest.mark.parametrize("sizes", [LADDER, LADDER[::-1], [(300, 400)] * 3 + [(1, 1)], [(2000, 2100), (5, 5)]])
def test_work_table_covers_every_step_once(sizes):
    recs, work, passes = B.colors_images_layout(_images(sizes))
    seen = [np.zeros(_ceil(h * w, STEP), np.int32) for h, w in sizes]
    for e in work:
        assert e["steps"] >= 1 and e["first_step"] >= 0
        assert e["first_step"] + e["steps"] <= len(seen[e["image"]])
        seen[e["image"]][e["first_step"]:e["first_step"] + e["steps"]] += 1
    assert all((s == 1).all() for s in seen)
    # a pass's entries are its images', in input order
    for p in passes:
        imgs = [e["image"] for e in work[p["work_first"]:p["work_first"] + p["work_count"]]]
        assert imgs == sorted(imgs) and set(imgs) == set(range(p["first"], p["first"] + p["count"]))


def _capacity(h, w):
    return L.lib().llfe_batch_capacity(h, w)


def test_pass_splitting_under_a_budget(monkeypatch):
    monkeypatch.setenv("LLFE_WORKSPACE_GB", "0.02")
    sizes = [(40, 50), (64, 64), (150, 96), (3, 5), (90, 160), (33, 31), (150, 96), (1, 1), (64, 64), (90, 160)]
    cap_big = _capacity(150, 96)
    assert 1 <= cap_big < len(sizes)  # (the budget really cuts this list)
    recs, _, passes = B.colors_images_layout(_images(sizes))
    assert len(passes) >= 2
    nxt = 0
    for k, p in enumerate(passes):  # contiguous, in input order
        assert p["first"] == nxt and p["count"] >= 1
        nxt += p["count"]
        members = sizes[p["first"]:p["first"] + p["count"]]
        big = max(members, key=lambda hw: hw[0] * hw[1])
        assert p["max_pixels"] == big[0] * big[1]
        assert p["count"] <= min(_capacity(*big), MAX_PASS)  # the budget rule, by the pass's largest image
        assert all(r["pass"] == k for r in recs[p["first"]:p["first"] + p["count"]])
    assert nxt == len(sizes)


def test_no_pass_exceeds_4096_images():
    one = np.zeros((1, 1, 3), np.uint8)
    recs, work, passes = B.colors_images_layout([one] * 9000)
    assert [p["count"] for p in passes] == [4096, 4096, 808]
    assert [p["first"] for p in passes] == [0, 4096, 8192]
    assert len(work) == 9000


def test_invalid_descriptors_are_refused():
    lib = L.lib()
    d = np.zeros(2, np.dtype(L.LlfeImageDesc))
    buf = np.zeros(64 * 3, np.uint8)
    d["data"], d["height"], d["width"] = buf.ctypes.data, 4, 4
    nw, npass = C.c_int64(0), C.c_int32(0)

    def plan(descs=d, n=2, mode=0):
        return lib.llfe_colors_images_layout(descs.ctypes.data if descs is not None else None, n, mode, None, None, 0,
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
    # a work table or a pass list that is too short
    work = (L.LlfeColorWork * 1)()
    assert lib.llfe_colors_images_layout(d.ctypes.data, 2, 0, None, work, 1, C.byref(nw), None, 0,
                                         C.byref(npass)) == L.LLFE_ERR_CAPACITY
    assert nw.value == 2


def test_abi_version_and_flag_bits():
    lib = L.lib()
    assert lib.llfe_abi_version() == 3
    assert C.sizeof(L.LlfeColorImage) == 48 and C.sizeof(L.LlfeColorWork) == 12 and C.sizeof(L.LlfeColorPass) == 64

    def call(flags):  # (no context: a flag word that passes its check goes on to the NULL-context refusal)
        return lib.llfe_process_images_flags(None, None, 0, 0, 0, 5, 0, 0, None, None, 0, None, None, flags)

    assert call(0) == L.LLFE_ERR_INVALID
    assert call(L.IMAGES_COLORS_ONE_PASS) == L.LLFE_ERR_INVALID
    for unknown in (2, 4, 1 << 31, 3):
        assert call(unknown) == L.LLFE_ERR_UNSUPPORTED, unknown


def test_colors_option_is_checked_without_a_gpu():
    from low_level_feature_extraction_amd.color_extractor import ColorExtractor
    from low_level_feature_extraction_amd.pipeline import run_batch

    assert B.colors_flags("grouped") == 0 and B.colors_flags("one_pass") == L.IMAGES_COLORS_ONE_PASS
    for bad in ("onepass", "", None, 1):
        with pytest.raises(ValueError):
            B.colors_flags(bad)
    imgs = _images([(4, 4), (5, 3)])
    with pytest.raises(ValueError):
        run_batch(imgs, ("colors",), colors="single")
    with pytest.raises(ValueError):
        ColorExtractor.extract_colors_batch(imgs, colors="single")
