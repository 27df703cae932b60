"""Lloyd's two-centre cubes walked 64 at a time from a per-wave list (kmeans.hip split_drain): in the
cells path a failing cube with exactly one contender is no longer split in its own batch; its index,
owner and contender wait in the wave's LDS list, a walk runs whenever 64 are pending, and one partial
walk per wave flushes the rest at the end of the sweep.  A list entry that is lost, walked twice or
decoded wrongly changes a count or a centre, so every case compares all 10 attempts of a small image, at
two seeds, with the oracle's cv2.kmeans restatement in its exact-sum mode: k-means++ centres,
iterations, float32 centres and counts equal, compactness within 1e-6 relative.

Every case also reads the attempt's LLFE_KM_TRACE line: the cubes split in place (column 17), the
walks that split them and the partial ones among those (the line's last two columns), and checks what
must hold whatever chunk a wave draws:

    split_partial <= KW x iterations    at most one flush per wave and sweep (KW = 8 waves in the
                                        512-thread build, which takes the batches whose attempts fit
                                        the GPU at once, 4 in the 256-thread build)
    64 (split_walks - split_partial) <= split_cubes <= 64 split_walks

The walk counts themselves depend on which wave draws which chunk and are not compared with
anything; the cube and colour counts do not, and are compared between runs.

Cases: the dense sweeps (`photo160`, `photo256`, `blobs_cells`); `rods`, where a bisector cuts all 64
cubes of a red quarter at once, so whole batches of 64 arrive on a wave's list -- on an empty one, and,
where the wave has drawn a partly cut quarter before, on one that already holds up to 63, which chunk a
wave draws being the device's choice (alone in the 512-thread build and as 104 copies in the
256-thread build, whose lists alias k-means++ state: 10 000 sweeps of four waves over eight chunks); `lattice`, one colour in each of the 2^18 cubes, so the entry's 18 index
bits are used to the top and every listed cube has a one-bit mask; `sparse`, whose sweeps hold fewer
than 64 two-centre cubes, so every walk is a flush; three images in one batch against each alone; and
both build widths on the same photos.  `ui160` (cubes-only sweep) never lists anything.
"""
import numpy as np
import pytest

from low_level_feature_extraction_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

K = 5
CELL_MIN = 8192  # kmeans.hip LLFE_KM_CELL_MIN
SEEDS = (2027, 31)
# LLFE_KM_TRACE columns (llfe_pipeline.cpp)
COL_ITERS, COL_LL_PTS, COL_SPLIT_CUBES, COL_SPLIT_PTS, COL_WALKS, COL_PARTIAL = 3, 15, 17, 18, 25, 26
KW_WIDE, KW_NARROW = 8, 4


def _image_of(rgb, side):
    """The colours `rgb` (n x 3, n <= side^2) as a side x side BGR image, padded with its first colour."""
    rgb = np.asarray(rgb, np.int64)
    assert len(rgb) <= side * side and rgb.min() >= 0 and rgb.max() <= 255, (len(rgb), side)
    full = np.concatenate([rgb, np.repeat(rgb[:1], side * side - len(rgb), 0)])
    return np.ascontiguousarray(full[:, ::-1].reshape(side, side, 3).astype(np.uint8))


def _blobs(edge, keep, side):
    """Two dense colour blobs (cubes of `edge`^3 colours, every `keep`-th colour present) and a
    thin line of colours that joins them through a corner of the colour space far from both."""
    rs = np.random.RandomState(5)
    ax = np.arange(edge)
    blk = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    blk = blk[rs.permutation(len(blk))[: len(blk) // keep]]
    a, b = blk + 24, blk + (232 - edge)
    n_line = side * side - 2 * len(blk)
    assert n_line > 0
    t = np.linspace(0.0, 1.0, n_line)[:, None]
    p0, p1, p2 = np.array([24.0 + edge, 24, 24]), np.array([250.0, 20, 128]), np.array([232.0 - edge, 232, 232])
    line = np.where(t < 0.5, p0 + (p1 - p0) * (2 * t), p1 + (p2 - p1) * (2 * t - 1))
    line = np.rint(line + rs.randint(-1, 2, line.shape)).clip(0, 255).astype(np.int64)
    rgb = np.concatenate([a, line, b])[rs.permutation(side * side)]
    return np.ascontiguousarray(rgb[:, ::-1].reshape(side, side, 3).astype(np.uint8))  # BGR


def _rods():
    """Two rods along the red axis, 256 x 32 x 32 colours each (8 x 8 cubes per red quarter: one 64-cube
    batch; 8 192 cubes in all), every cube's origin colour and a twelfth of the rest present.  Two
    centres of one rod differ mostly in red, so their bisector is nearly perpendicular to the red axis
    and cuts every cube of a red quarter at once: batches of exactly 64 two-centre cubes, beside the
    partly cut quarters of the tilted bisectors (the first sweeps'), which leave a list non-empty."""
    rs = np.random.RandomState(5)
    blk = np.stack(np.meshgrid(np.arange(256), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)
    corner = ((blk & 3) == 0).all(1)
    out = []
    for o in (32, 192):
        rest = blk[~corner][rs.permutation(int((~corner).sum()))[: len(blk) // 12]]
        out.append(np.concatenate([blk[corner], rest]) + np.array([0, o, o]))
    return _image_of(np.concatenate(out), 228)


def _lattice():
    """512 x 512 pixels, one colour in each of the 64^3 = 2^18 cubes (a position that varies from cube to
    cube): the largest cube table there is, every occupancy mask has one bit."""
    ax = np.arange(64)
    c = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    u = np.stack([(c[:, 0] + c[:, 1]) & 3, (c[:, 1] + 2 * c[:, 2]) & 3, (c[:, 2] + 3 * c[:, 0] + 1) & 3], 1)
    rs = np.random.RandomState(11)
    return _image_of((c * 4 + u)[rs.permutation(len(c))], 512)


def _sparse():
    """Five compact blobs far from each other, 12^3 cubes each with the cube's origin colour and a few
    more (8 640 cubes: the cells path), joined by thin lines of colours.  With a centre in each blob the
    bisectors run through empty space and cut only the lines: a handful of two-centre cubes per sweep."""
    rs = np.random.RandomState(3)
    ax = np.arange(12) * 4
    o = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    corners = np.array([(4, 4, 4), (204, 4, 4), (4, 204, 204), (204, 204, 4), (104, 104, 204)])
    pts = []
    for cr in corners:
        pts.append(o + cr)
        pts.append(o[rs.permutation(len(o))[:600]] + cr + rs.randint(1, 4, (600, 3)))
    for a, b in zip(corners[:-1], corners[1:]):
        t = np.linspace(0.0, 1.0, 180)[:, None]
        pts.append(np.rint(a + 24 + (b - a) * t).astype(np.int64))
    return _image_of(np.concatenate(pts), 112)


# name -> (image, production noise (False: zero noise, the colours are exactly the image's), cells path)
CASES = {
    "photo160": (lambda: synth.synth_numpy(1, 160, 160, seed=2025), True, True),
    "photo256": (lambda: synth.synth_numpy(1, 256, 256, seed=2025), True, True),
    "blobs_cells": (lambda: _blobs(64, 4, 384), True, True),
    "rods": (_rods, False, True),
    "lattice": (_lattice, False, True),
    "sparse": (_sparse, False, True),
    "ui160": (lambda: synth.synth_numpy(0, 160, 160, seed=2025), True, False),  # cubes-only sweep: no lists
}


def _read_trace(path):
    return np.atleast_2d(np.loadtxt(path, dtype=np.int64))


def _check_counters(t, kw, cells, tag):
    """The identities every attempt's counters satisfy (rows of the trace `t`)."""
    assert t.shape[1] > COL_PARTIAL, (tag, t.shape)
    for a, row in enumerate(t):
        iters, cubes, walks, part = (int(row[c]) for c in (COL_ITERS, COL_SPLIT_CUBES, COL_WALKS, COL_PARTIAL))
        assert 0 <= part <= walks, (tag, a, walks, part)
        assert part <= kw * iters, (tag, a, part, kw, iters)
        assert 64 * (walks - part) <= cubes <= 64 * walks, (tag, a, cubes, walks, part)
        if not cells:
            assert walks == 0 and cubes == 0 and int(row[COL_SPLIT_PTS]) == 0, (tag, a, walks, cubes)


def _check_attempts(att, ex, tag):
    for a in range(10):
        assert np.array_equal(att[a]["pp_centers"][:K], ex["pp"][a]), (tag, a, att[a]["pp_centers"], ex["pp"][a])
        assert att[a]["iters"] == int(ex["iters"][a]), (tag, a, att[a]["iters"], ex["iters"][a])
        assert np.array_equal(att[a]["centers"][:K], ex["att_centers"][a]), (tag, a)
        assert np.array_equal(att[a]["counts"][:K], ex["att_counts"][a]), (tag, a)
        assert abs(att[a]["compactness"] - ex["att_compactness"][a]) <= 1e-6 * ex["att_compactness"][a], (tag, a)


def _n_cubes(keys):
    return len(np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63)))


@pytest.fixture(scope="module")
def images():
    return {name: make() for name, (make, _, _) in CASES.items()}


@pytest.fixture(scope="module")
def runs(orc, images):
    """name, seed -> (noise or None, unique keys, the oracle's attempts); computed once"""
    out = {}
    for name, host in images.items():
        h, w = host.shape[:2]
        for seed in SEEDS:
            noise = None if CASES[name][1] else np.zeros((h * w, 3), np.int8)
            keys = orc.color_unique(host, orc.device_noise(h * w, seed, 0) if noise is None else noise)
            out[name, seed] = (noise, keys, orc.kmeans_attempts(keys, K, orc.image_rng_state(seed, 0), exact_sums=True))
    return out


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", list(CASES))
def test_attempts_equal_exact_sum_oracle(backend, images, runs, tmp_path, monkeypatch, name, seed):
    host = images[name]
    noise, keys, ex = runs[name, seed]
    trace = tmp_path / "km_trace.txt"
    monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
    r = backend.process(host[None], ("colors",), seed=seed, index_base=0, noise=noise)[0]
    att = backend.kmeans_attempts(1)[0]
    assert r.n_unique == len(keys)
    cells = CASES[name][2]
    n_cubes = _n_cubes(keys)
    assert (n_cubes >= CELL_MIN) == cells, (name, n_cubes)
    t = _read_trace(trace)
    assert t.shape[0] == 10, t.shape
    tot = {c: int(t[:, c].sum()) for c in (COL_ITERS, COL_LL_PTS, COL_SPLIT_CUBES, COL_SPLIT_PTS, COL_WALKS, COL_PARTIAL)}
    print(f"{name} seed {seed}: U={len(keys)} cubes={n_cubes} sweeps={tot[COL_ITERS] - 10} split cubes={tot[COL_SPLIT_CUBES]}"
          f" colours decided={tot[COL_SPLIT_PTS]} walks={tot[COL_WALKS]} (partial {tot[COL_PARTIAL]}),"
          f" live lanes per walk {tot[COL_SPLIT_CUBES] / max(tot[COL_WALKS], 1):.1f}, labelled one by one={tot[COL_LL_PTS]}")
    _check_attempts(att, ex, name)
    _check_counters(t, KW_WIDE, cells, name)  # (one image: 10 attempts, the 512-thread build)
    if cells:
        assert tot[COL_SPLIT_CUBES] > 0 and tot[COL_WALKS] > 0, (name, tot)
    if name == "lattice":
        assert n_cubes == 1 << 18 and len(keys) == 1 << 18, (n_cubes, len(keys))
        # one colour per cube: a walked cube decides at most its one colour
        assert tot[COL_SPLIT_PTS] <= tot[COL_SPLIT_CUBES], tot
    if name == "rods":
        # whole batches of 64 arrive: far more full walks than flushes
        assert tot[COL_WALKS] - tot[COL_PARTIAL] > 0, tot
    if name == "sparse":
        # an attempt whose sweeps never fill a list: every walk it ran was a flush
        flush_only = [a for a in range(10) if t[a, COL_WALKS] > 0 and t[a, COL_WALKS] == t[a, COL_PARTIAL]]
        assert flush_only, t[:, [COL_WALKS, COL_PARTIAL]].tolist()


def test_rods_in_the_narrow_build(backend, images, runs, tmp_path, monkeypatch):
    """104 copies of `rods` in one batch (1 040 attempts: the 256-thread build, whose lists alias the
    k-means++ partition sums): image 0 equals the oracle, every attempt's counters satisfy the identities."""
    host = images["rods"]
    seed = SEEDS[0]
    _, keys, ex = runs["rods", seed]
    n = 104
    trace = tmp_path / "km_trace.txt"
    monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
    batch = np.ascontiguousarray(np.broadcast_to(host, (n,) + host.shape))
    r = backend.process(batch, ("colors",), seed=seed, index_base=0, noise=np.zeros((n * host.shape[0] * host.shape[1], 3), np.int8))
    att = backend.kmeans_attempts(n)
    assert all(x.n_unique == len(keys) for x in r)
    _check_attempts(att[0], ex, "rods x 104")
    t = _read_trace(trace)
    assert t.shape[0] == 10 * n, t.shape
    _check_counters(t, KW_NARROW, True, "rods x 104")
    print(f"rods x {n}: split cubes={int(t[:, COL_SPLIT_CUBES].sum())} walks={int(t[:, COL_WALKS].sum())}"
          f" (partial {int(t[:, COL_PARTIAL].sum())})")
    assert (t[:, COL_WALKS] > t[:, COL_PARTIAL]).any()


def test_images_of_a_batch_equal_each_alone(backend, tmp_path, monkeypatch):
    """Three different cells-path images in one batch: the results and the cube / colour counters of
    images 1 and 2 (whose cube tables start at a stride, not at 0) equal those of each run alone under
    its own index."""
    imgs = np.stack([synth.synth_numpy(2 * i + 1, 160, 160, seed=2025) for i in range(3)])
    cols = [COL_ITERS, COL_LL_PTS, COL_SPLIT_CUBES, COL_SPLIT_PTS]

    def run(batch, base, tag):
        trace = tmp_path / f"km_trace_{tag}.txt"
        monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
        res = backend.process(batch, ("colors",), seed=77, index_base=base)
        att = backend.kmeans_attempts(len(batch))
        t = _read_trace(trace)
        assert t.shape[0] == 10 * len(batch), (tag, t.shape)
        _check_counters(t, KW_WIDE, True, tag)
        return res, att, t

    res3, att3, t3 = run(imgs, 0, "three")
    for i in (1, 2):
        res1, att1, t1 = run(imgs[i:i + 1], i, f"alone{i}")
        assert res3[i].n_unique == res1[0].n_unique, i
        assert np.array_equal(np.asarray(res3[i].centers_rgb), np.asarray(res1[0].centers_rgb)), i
        assert np.array_equal(np.asarray(res3[i].counts), np.asarray(res1[0].counts)), i
        assert res3[i].compactness == res1[0].compactness, i
        for a in range(10):
            for f in ("pp_centers", "centers", "counts"):
                assert np.array_equal(att3[i][a][f], att1[0][a][f]), (i, a, f)
            assert att3[i][a]["iters"] == att1[0][a]["iters"] and att3[i][a]["compactness"] == att1[0][a]["compactness"], (i, a)
        rows = t3[t3[:, 0] == i]
        rows = rows[np.argsort(rows[:, 1])]
        alone = t1[np.argsort(t1[:, 1])]
        assert np.array_equal(rows[:, cols], alone[:, cols]), (i, rows[:, cols].tolist(), alone[:, cols].tolist())
        assert int(rows[:, COL_SPLIT_CUBES].sum()) > 0 and int(rows[:, COL_WALKS].sum()) > 0, i


def test_both_build_widths_split_and_agree(backend, tmp_path, monkeypatch):
    """104 photos of 160 x 160 as one batch (1 040 attempts: the 256-thread build) and its first 2 as a
    batch of 2 (20 attempts: the 512-thread build), same indices and seed: both walk their lists, the
    results and the cube / colour counters are equal."""
    big = np.stack([synth.synth_numpy(2 * i + 1, 160, 160, seed=2025) for i in range(104)])
    cols = [COL_ITERS, COL_LL_PTS, COL_SPLIT_CUBES, COL_SPLIT_PTS]
    out = []
    for tag, batch, kw in (("wide", big[:2], KW_WIDE), ("narrow", big, KW_NARROW)):
        trace = tmp_path / f"km_trace_{tag}.txt"
        monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
        res = backend.process(batch, ("colors",), seed=77, index_base=0)[:2]
        t = _read_trace(trace)
        assert t.shape[0] == 10 * len(batch), (tag, t.shape)
        _check_counters(t, kw, True, tag)
        t = t[t[:, 0] < 2]
        t = t[np.lexsort((t[:, 1], t[:, 0]))]
        print(f"{tag}: split cubes {int(t[:, COL_SPLIT_CUBES].sum())}, walks {int(t[:, COL_WALKS].sum())}"
              f" (partial {int(t[:, COL_PARTIAL].sum())})")
        assert int(t[:, COL_WALKS].sum()) > 0 and int(t[:, COL_SPLIT_CUBES].sum()) > 0, tag
        out.append((res, t[:, cols]))
    (ra, ta), (rb, tb) = out
    assert np.array_equal(ta, tb)
    for i, (a, b) in enumerate(zip(ra, rb)):
        assert a.n_unique == b.n_unique, i
        assert np.array_equal(np.asarray(a.centers_rgb), np.asarray(b.centers_rgb)), i
        assert np.array_equal(np.asarray(a.counts), np.asarray(b.counts)), i
        assert a.compactness == b.compactness, i
