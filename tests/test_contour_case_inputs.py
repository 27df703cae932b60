"""What the masks of tests/contour_cases.py reach, asserted on the CPU.

tests/test_gpu_contour_cases.py runs these masks through the GPU contour path; a case is only
worth its GPU time while it still reaches the branch it is named for.  Here every such claim
is an assertion, from the host library (``backend.find_contours``, no GPU), the oracle and
8-connected labelling alone: how many components the scan rejects, how long the borders are,
which columns are empty, which first pixels start a border.  The same counters are applied
to the inputs of tests/test_gpu_contours.py, so DESIGN.md's table of what the older tests do and
do not reach stays true.  The file also holds the exhaustive small-mask search for a border
that starts away from a component's first pixel, and the Douglas-Peucker depth record.
"""
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from low_level_feature_extraction_amd import backend as B
from tests import contour_cases as cc


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def contours(orc):
    """name -> the oracle's contours of the case, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = orc.find_contours_external(cc.SINGLE[name]())
        return cache[name]

    return get


def _starts(cs):
    return {(int(c[0][0]), int(c[0][1])) for c in cs}


def _rejected_first_pixels(mask, cs):
    """first pixels of the rejected components, in raster order, as (x, y)"""
    return sorted(cc.first_pixels(mask) - _starts(cs), key=lambda p: (p[1], p[0]))


# ------------------------------------------------------------------ every case
@pytest.mark.parametrize("name", sorted(cc.SINGLE))
def test_host_library_and_oracle_agree_and_borders_start_at_first_pixels(contours, name):
    m = cc.SINGLE[name]()
    cs = contours(name)
    assert _same(B.find_contours(m), cs)
    c = cc.counters(m, cs)
    # a contour that does not start at its component's first pixel would be an input for the
    # Q planes of k_ct_scan, which no known mask reaches
    assert c["off_first"] == 0
    assert len(_starts(cs)) == len(cs)
    if name in cc.REJECTED:
        assert c["rejected"] == cc.REJECTED[name]
    elif name.startswith(("wide_rej_", "far_")):
        assert c["rejected"] >= 1
    else:
        assert c["rejected"] == 0
    assert m.shape[0] <= 48 or not name.startswith(("rej_", "wide_", "far_", "restarts"))


# ------------------------------------------------------------------ A1
def _behind_a_bar(m, rej):
    """rejected dots with the second row of a rejected two-row component 3 px to their left:
    what a live mark of that component would wrongly accept"""
    lab, _ = cc.components(m)
    rejected = {int(lab[y, x]) for x, y in rej}
    out = []
    for x, y in rej:
        left = np.nonzero(m[y, :x])[0]
        if len(left) and x - int(left[-1]) == 3 and m[y - 1, left[-1]] and int(lab[y, left[-1]]) in rejected \
                and lab[y - 1, left[-1]] == lab[y, left[-1]]:
            out.append((x, y))
    return out


def test_rej_grid_passes_the_box_limit_before_the_block_starts(contours):
    m = cc.rej_grid()
    rej = _rejected_first_pixels(m, contours("rej_grid"))
    assert len(rej) == 462 > cc.REJ_BOXES
    block_row = int(np.nonzero(m[:, 130])[0][0])
    assert rej[cc.REJ_BOXES][1] < block_row          # the 65th rejection
    assert (125, block_row) in _starts(contours("rej_grid"))
    behind = _behind_a_bar(m, rej)
    assert len(behind) == 154
    assert sum(p[1] > rej[cc.REJ_BOXES][1] for p in behind) >= 126   # ... nine of eleven rows past the limit


@pytest.mark.parametrize("n", [64, 65, 66])
def test_rej_n_counts(contours, n):
    m = cc.rej_n(n)
    rej = _rejected_first_pixels(m, contours(f"rej_{n}"))
    assert len(rej) == n and len(contours(f"rej_{n}")) == 2
    behind = _behind_a_bar(m, rej)
    assert len([p for p in behind if rej.index(p) < cc.REJ_BOXES]) >= 14     # behind components that have a box
    if n >= 65:     # the first component without a box has two rows
        x, y = rej[64]
        assert m[y + 1, x] and not m[y + 2, x]
    if n == 66:     # ... and the 66th is the dot behind its second row
        assert rej[65] == (rej[64][0] + 3, rej[64][1] + 1) and rej[65] in behind


@pytest.mark.parametrize("many", [False, True])
def test_rej_straddle_components_cross_the_word_edge(contours, many):
    name = "rej_straddle_many" if many else "rej_straddle_few"
    m = cc.rej_straddle(many)
    lab, _ = cc.components(m)
    started = {int(lab[y, x]) for x, y in _starts(contours(name))}
    crossing = {int(l) for l in np.unique(lab[:, 63]) if l and l in np.unique(lab[:, 64])} - started
    assert len(crossing) == 3                        # two blocks and a 2x2 blob, all rejected
    rej = _rejected_first_pixels(m, contours(name))
    assert (63, 33) in rej and m[33:35, 63:65].all() and not m[32:36, 62].any() and not m[32:36, 65].any()
    dots = [p for p in _behind_a_bar(m, rej) if p[1] >= 27]
    assert len(dots) == 3 and all(p[0] > 64 for p in dots)
    # in raster order the straddling components come after the 64th rejection, or before it
    first_cross = min(i for i, p in enumerate(rej) if int(lab[p[1], p[0]]) in crossing)
    assert (first_cross > cc.REJ_BOXES) == many


# ------------------------------------------------------------------ A2
@pytest.mark.parametrize("w", cc.WIDE)
def test_wide_rej_rejections_in_the_second_window(contours, w):
    m = cc.wide_rej(w)
    assert m.shape == (15, w)
    rej = _rejected_first_pixels(m, contours(f"wide_rej_{w}"))
    assert len(rej) >= 5 and len(contours(f"wide_rej_{w}")) == 1
    behind = _behind_a_bar(m, rej)
    second = [p for p in rej if p[0] >= cc.WIN0]
    if w == 4033:
        # a hole needs a wall to its right: no first pixel of the last column can be rejected,
        # the second window holds the ring's right wall and nothing else
        assert not second and m[1:14, cc.WIN0].all()
        assert sorted(p[0] for p in behind) == [3968, 4023, 4030]    # in and over the window's lane-0 word
    else:
        assert len(second) >= 8
        assert len([p for p in behind if p[0] - 3 >= cc.WIN0]) == 4          # bar and dot inside the second window
        assert sorted(p[0] for p in behind if p[0] - 3 < cc.WIN0) == [4033, 4034]   # bar left of 4032, dot right of it


# ------------------------------------------------------------------ A3
@pytest.mark.parametrize("w", cc.WIDE)
def test_far_rows_are_what_they_say(contours, w):
    m = cc.far(w)
    cs = contours(f"far_{w}")
    fp, started = cc.first_pixels(m), _starts(cs)
    rows = cc.far_rows(w)
    assert len(rows) == (4 if w == 4033 else 8)
    for y, (qx, starts, last) in rows.items():
        assert qx >= cc.WIN0 and (qx, y) in fp, y
        left = np.nonzero(m[y, :qx])[0]
        if last is None:
            assert not len(left), y
        else:
            assert int(left[-1]) == last, y
            # nothing between the lnbd candidate and the query, so the scan has to look outside
            # the window (last < 3968) or into its lane-0 word (last == 3968)
            assert last <= cc.LANE0 < cc.WIN0 <= qx
        assert ((qx, y) in started) == starts, y
    if w != 4033:
        lab, _ = cc.components(m)
        assert (3900, 9) in fp and (3900, 9) not in started     # (b): the dot before the query is rejected
        assert lab[9, 3800] == lab[7, 3800] and (3800, 7) in started   # (b), (c): the wall is an accepted ring's
    assert cc.far_lookups(m) == (2 if w == 4033 else 5)


# ------------------------------------------------------------------ A4
def test_restart_rows_alternate_accepted_and_rejected_first_pixels(contours):
    m = cc.restarts()
    fp, started = cc.first_pixels(m), _starts(contours("restarts"))
    words = []
    for k in range(len(cc.RESTART_PHASES)):
        y, xs = cc.restart_row_pixels(k)
        assert [x for x in range(m.shape[1]) if (x, y) in fp] == list(xs)   # the row's first pixels, no others
        assert [(x, y) in started for x in xs] == [True, False, True, False]
        words.append([x // 64 for x in xs])
    assert words[0] == [0, 0, 0, 0]
    assert words[1] == [0, 0, 0, 1] and words[2] == [0, 0, 0, 1] and words[3] == [0, 0, 1, 1]
    assert cc.restart_row_pixels(2)[1][2] == 62 and cc.restart_row_pixels(3)[1][1] == 62


# ------------------------------------------------------------------ B5
@pytest.mark.parametrize("ph,pw", [(3, 4), (4, 3)])
def test_corner_batches_hold_every_pattern_and_one_kept_shape_each(orc, ph, pw):
    m = cc.corners(ph, pw)
    assert m.shape == (4096, 64, 128)
    y0, x0 = cc.CORNER_Y - 2, cc.CORNER_X - 2
    pat = m[:, y0:y0 + ph, x0:x0 + pw].reshape(4096, -1) != 0
    assert y0 < cc.CORNER_Y < y0 + ph and x0 < cc.CORNER_X < x0 + pw
    assert len(np.unique(pat @ (1 << np.arange(ph * pw)))) == 4096
    rest = m.copy()
    rest[:, y0:y0 + ph, x0:x0 + pw] = 0
    assert not rest[:, 14:, :].any() and not rest[:, :, 21:].any()       # the block stays in tile (0, 0)
    for i in range(0, 4096, 37):
        cs = orc.find_contours_external(m[i])
        assert _same(B.find_contours(m[i]), cs)
        c = cc.counters(m[i], cs)
        assert c["rejected"] == 0 and c["off_first"] == 0
        assert sum(orc.contour_area(c) >= 100 for c in cs) == 1


# ------------------------------------------------------------------ B6
@pytest.mark.parametrize("h,w", cc.SIZES)
def test_first_pixel_is_far_from_the_body(contours, h, w):
    m = cc.serpentine(h, w)
    (x, y), = cc.first_pixels(m)
    assert x // cc.TW == (w - 1) // cc.TW and y == 0
    tiles = {(yy // cc.TH, xx // cc.TW) for yy, xx in zip(*np.nonzero(m))}
    assert len(tiles) == -(-h // cc.TH) * -(-w // cc.TW)         # one component through every tile
    for d in ("ne", "nw", "se", "sw"):
        m = cc.corner_link(h, w, d)
        _, k8 = cc.components(m)
        from scipy import ndimage
        _, k4 = ndimage.label(m != 0)
        assert (k8, k4) == (1, 2), d                             # one diagonal contact holds it together
        q = m[cc.CORNER_Y - 1:cc.CORNER_Y + 1, cc.CORNER_X - 1:cc.CORNER_X + 1] != 0
        assert q.tolist() == ([[False, True], [True, False]] if d in ("ne", "sw") else [[True, False], [False, True]])
        (x, y), = cc.first_pixels(m)
        if d in ("ne", "nw"):   # the raster-first pixel is the lone one, alone in its tile
            ty, tx = y // cc.TH, x // cc.TW
            assert (m[ty * cc.TH:(ty + 1) * cc.TH, tx * cc.TW:(tx + 1) * cc.TW] != 0).sum() == 1


# ------------------------------------------------------------------ B7
@pytest.mark.parametrize("name", ["spiral", "diagonal", "staircase", "window_edge"])
def test_thin_curves_leave_the_tracer_window_and_are_kept(orc, contours, name):
    m = cc.SINGLE[name]()
    assert m.shape == (200, 300)
    (c,) = contours(name)
    assert orc.contour_area(c) >= 100
    assert np.ptp(c[:, 1]) + 1 >= 2 * 64      # the tracer's window holds 64 rows around its centre
    if name == "window_edge":
        for y in (63, 64):
            assert (m[y, 20:257] != 0).sum() >= 100
        for x in (255, 256):
            assert (m[63:191, x] != 0).sum() >= 60


# ------------------------------------------------------------------ B8, B9
@pytest.mark.parametrize("name", sorted(cc.COMBS))
def test_comb_vertex_counts(orc, contours, name):
    (c,) = contours(name)
    assert len(c) == cc.COMBS[name][2]
    assert orc.contour_area(c) >= 100


def test_comb_counts_sit_on_the_thresholds():
    n = {k: v[2] for k, v in cc.COMBS.items()}
    assert n["comb_a"] == cc.PTS_LDS < n["comb_b"] <= cc.PTS_LDS + 2
    assert n["comb_c"] == cc.STAGE < n["comb_d"] <= cc.STAGE + 2
    assert 12000 < n["comb_e"] < 14000


def test_regrow_has_more_vertices_than_the_default_pool(contours):
    cs = contours("regrow")
    assert len(cs) == 15 and {len(c) for c in cs} == {5862}
    assert sum(len(c) for c in cs) == 87930 > cc.PTS_DEFAULT_1 == 81920


# ------------------------------------------------------------------ Douglas-Peucker depth
def test_douglas_peucker_stays_far_from_its_capacities(orc, contours):
    """kDpStack = 512 pairs and kDpOut = 1024 points.  Kept points are about eps = 0.02 x
    perimeter apart, so a closed contour keeps a few dozen at most: over every kept contour of
    the new cases the restated iteration needs 3 stack pairs and emits 4 points at the most
    (a long thin border has a huge perimeter and so a huge eps); the bound asserted below still
    leaves a factor of 8 to the capacities."""
    deepest = most = 0
    for name in cc.SINGLE:
        for c in contours(name):
            if orc.contour_area(c) < 100:
                continue
            per = orc.arc_length(c, True)
            for k in (0.02, 0.04):
                d, n, final = cc.dp_depth(c, k * per)
                assert final == len(orc.approx_poly_dp(c, k * per, True)), (name, k)   # the restatement is right
                deepest, most = max(deepest, d), max(most, n)
    print("Douglas-Peucker over the contour cases: stack depth", deepest, "pairs, output", most, "points")
    assert 0 < deepest <= 512 // 8 and 0 < most <= 1024 // 8


# ------------------------------------------------------------------ the older inputs
def _older_inputs(orc):
    from low_level_feature_extraction_amd.synth import synth_numpy
    from tests.test_gpu_contours import MASKS

    out = dict(MASKS)
    for kind, seed in (("ui", 0), ("ui", 1), ("ui", 2), ("photo", 3)):
        out[f"1080p_{kind}_{seed}"] = orc.shape_mask(synth_numpy(seed, 1080, 1920, kind=kind))
    return out


def test_what_the_older_inputs_reach(orc):
    """The table of DESIGN.md section 5: none of the masks of tests/test_gpu_contours.py fills the
    rejection boxes, follows a border twice or overflows the vertex pool; only two of the 1080p
    masks have a contour that k_ct_shapes reads from global memory."""
    rows = {}
    for name, m in _older_inputs(orc).items():
        cs = orc.find_contours_external(m)
        rows[name] = cc.counters(m, cs)
        rows[name]["far"] = cc.far_lookups(m) if m.shape[1] > cc.WIN0 else 0
    assert max(r["rejected"] for r in rows.values()) == rows["half"]["rejected"] == 26 < cc.REJ_BOXES
    assert rows["wide_4096"]["rejected"] == rows["wide_4033"]["rejected"] == 0
    assert (rows["wide_4096"]["far"], rows["wide_4033"]["far"]) == (1, 0)
    named = {k: r for k, r in rows.items() if not k.startswith("1080p")}
    assert max(r["longest"] for r in named.values()) == rows["half"]["longest"] == 980 < cc.PTS_LDS
    assert [rows[f"1080p_{k}"]["longest"] for k in ("ui_0", "ui_1", "ui_2", "photo_3")] == [1097, 3406, 569, 0]
    assert max(r["longest"] for r in rows.values()) < cc.STAGE
    assert max(r["vertices"] for r in rows.values()) == 15900 < cc.PTS_DEFAULT_1
    assert all(r["off_first"] == 0 for r in rows.values())


# ------------------------------------------------------------------ exhaustive small masks
@pytest.mark.parametrize("h,w", [(4, 4), (3, 5)])
def test_every_small_mask_starts_every_border_at_a_first_pixel(h, w):
    """Every h x w mask through the host library: its contours are its 8-connected components,
    one each, and each starts at its component's raster-first pixel.  (A hole of such a mask has
    no room for a second component, so nothing is rejected either.)  With the 3x6, 4x5, 5x4 and
    3x7 enumerations made for DESIGN.md this covers every mask of up to 21 pixels: no input is
    known for the borders k_ct_scan follows itself."""
    from scipy import ndimage

    lib = L.lib()
    n = 1 << (h * w)
    idx = np.arange(n, dtype=np.uint32)
    masks = np.zeros((n, h, w), np.uint8)
    for b in range(h * w):
        masks[:, b // w, b % w] = (idx >> b) & 1
    # reference, all masks at once: stacked with an empty row between them
    tall = np.zeros((n, h + 1, w), np.uint8)
    tall[:, :h] = masks
    lab, k = ndimage.label(tall.reshape(-1, w), structure=np.ones((3, 3)))
    pos = ndimage.minimum(np.arange(lab.size).reshape(lab.shape), lab, np.arange(1, k + 1)).astype(np.int64)
    first = [set() for _ in range(n)]
    for p in pos:
        y, x = divmod(int(p), w)
        first[y // (h + 1)].add((x, y % (h + 1)))
    pts = np.empty((4 * h * w, 2), np.int32)   # a thin line's pixels are vertices on the way out and back
    offs = np.empty(h * w + 2, np.int32)
    need = C.c_int64(0)
    for i in range(n):
        nc = lib.llfe_find_contours(masks[i].ctypes.data, h, w, pts.ctypes.data, len(pts), offs.ctypes.data, len(offs),
                                    C.byref(need))
        starts = {(int(pts[offs[j], 0]), int(pts[offs[j], 1])) for j in range(nc)}
        assert nc == len(first[i]) and starts == first[i], (i, nc)


@pytest.mark.parametrize("h,w", [(3, 6), (4, 5)])
def test_every_larger_small_mask_stacked(h, w):
    """The same property for every 3x6 and 4x5 mask, 2^18 masks per call: stacked into one tall
    image with an empty row between them.  The scan's state (lnbd) starts afresh on every row and
    a border never crosses an empty row, so the masks cannot influence each other.  Run once
    with (5, 4), (3, 7), (7, 3), (2, 11) and (11, 2) as well (every mask of up to 22 pixels;
    half a minute), with the same result: DESIGN.md section 3."""
    from scipy import ndimage

    n, step = 1 << (h * w), 1 << 18
    for c0 in range(0, n, step):
        idx = np.arange(c0, min(n, c0 + step), dtype=np.uint32)
        tall = np.zeros((len(idx), h + 1, w), np.uint8)
        for b in range(h * w):
            tall[:, b // w, b % w] = (idx >> b) & 1
        img = tall.reshape(-1, w)
        lab, k = ndimage.label(img, structure=np.ones((3, 3)))
        first = ndimage.minimum(np.arange(lab.size).reshape(lab.shape), lab, np.arange(1, k + 1)).astype(np.int64)
        starts = np.array([int(c[0][1]) * w + int(c[0][0]) for c in B.find_contours(img)], np.int64)
        assert len(starts) == k and np.array_equal(np.sort(starts), np.sort(first)), c0
