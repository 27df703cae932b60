"""CPU preconditions of tests/stencil_cases.py: the shapes reach the ring phases and strip
kinds its table claims, and the images put pixels on every threshold and NMS tie (oracle
stages only).  The device runs the same shapes in tests/test_gpu_stencil_seams.py."""
import numpy as np

from tests import stencil_cases as SC

TIES = ("m50", "m52", "m150", "m152", "left", "right", "up", "down", "diag_ul", "diag_dr", "diag_ur", "diag_dl",
        "shadow1", "shadow2")


def test_geometry_restates_the_kernel_launch():
    assert SC.geometry(1080, 1920) == (8, 5, 216)
    assert SC.geometry(270, 480) == (2, 2, 135)
    assert SC.geometry(257, 3) == (1, 2, 129)
    assert [SC.geometry(h, 12)[1] for h in (432, 433, 434, 648, 649)] == [2, 3, 3, 3, 4]
    assert SC.geometry(215, 12)[1] == SC.geometry(216, 12)[1] == 1
    assert [SC.geometry(h, 12)[2] for h in range(217, 241)] == [109 + k // 2 for k in range(24)]


def test_g3_covers_every_ring_phase():
    starts = set()
    for h, w in SC.G3:
        _, segs, seg_rows = SC.geometry(h, w)
        starts |= {(s * seg_rows) % 12 for s in range(1, segs)}
    assert starts == set(range(12))
    assert {h % 12 for h, _ in SC.G3} == set(range(12))
    # ... and G4 puts a `fast` wave on a seam at a phase the older tests never start at
    for h, w in SC.G4:
        _, segs, seg_rows = SC.geometry(h, w)
        assert segs >= 2 and SC.fast_strips(w) and seg_rows % 12 not in (0, 3, 9)


def test_488_is_the_first_width_with_a_fast_strip():
    assert all(not SC.fast_strips(w) for w in range(1, 488))
    assert SC.fast_strips(488) == [1] and SC.fast_strips(728) == [1, 2] and SC.fast_strips(724) == [1]
    widths = {w for _, w in SC.G2}
    assert {1, 4, 8, 12} <= {w - 240 for w in widths if 240 < w <= 252}  # last strips of 1 .. 12 columns
    assert {240, 480, 720} <= widths


def test_batches_leave_a_partial_workgroup():
    for h, w in SC.FIVE:
        strips, segs, _ = SC.geometry(h, w)
        assert len(SC.images(h, w)) == 5 and (5 * strips * segs) % 4
    assert len(SC.images(13, 240)) == 3
    assert SC.PROCESS <= set(SC.SHAPES) and SC.FIVE <= set(SC.SHAPES)


def test_magnitudes_are_even_and_blocks_reach_every_tie():
    """|dx| + |dy| = dx + dy = 2 (p22 - p00) (mod 2): no pixel at 51 or 151, so the threshold
    ties are 50 | 52 and 150 | 152.  The counts measured on blocks are in DESIGN.md (Parity)."""
    small = SC.tie_counts(SC.blocks(61, 244, 0))
    big = SC.tie_counts(SC.blocks(229, 244, 0))
    print("blocks 61x244", small)
    print("blocks 229x244", big)
    assert small["odd"] == 0 and big["odd"] == 0
    for k in TIES:
        assert small[k] >= 20, (k, small[k])
        assert big[k] >= 100, (k, big[k])  # (the diagonal ties are the rarest: 106 .. 152)


def test_seam_image_set_reaches_every_tie_and_large_magnitudes():
    total = dict.fromkeys(TIES, 0)
    top = 0
    for h, w in SC.G2 + SC.G4 + tuple(s for s in SC.G3 if s[0] in (217, 229, 433)):
        x = SC.images(h, w)
        for i, img in enumerate(x):
            t = SC.tie_counts(img)
            assert t["odd"] == 0
            for k in TIES:
                total[k] += t[k]
            if i % 3 == 1 or i == 4:  # the saturated images
                top = max(top, t["max"])
    print("G2-G4", total, "max m", top)
    for k in TIES:
        assert total[k] >= 20, (k, total[k])
    assert 800 <= top <= 2040  # the packed 12-bit magnitude field holds 4 * 2 * 255
