"""k-means++ split of owned straddling cubes (kmeans.hip split_owned / gain_signs): a cube that one
chosen centre c_k owns and on which a trial t is neither never nor always closer is summed in
place, the trial's gain being the exact integer form G(u) = d(o + u, c_k) - d(o + u, t) over the
positions with G > 0 (one lane per cube, 64 positions in a bit mask).  A gain that is off by one
changes a choice of centre somewhere across 10 attempts x 4 rounds x 2 seeds, so every case runs
the device on one small image and compares all 10 attempts with the oracle's cv2.kmeans
restatement in its exact-sum mode: k-means++ centres, iterations, float32 centres and counts
equal, compactness within 1e-6 relative.

The last two columns of an attempt's LLFE_KM_TRACE line carry the cubes k-means++ split in place
and their colours, column 11 the colours it still summed one by one.  What each case expects of
them comes from the NumPy model of the sweeps' batches (tools/km_pp_gain_sim.py attempts_split)
run on the exact unique colours and RNG stream of the case, not from the device: the model forms
the 64-cube batches as the kernel does (cells path: the cubes of a 64-cell batch's failing cells
per partition, split from LLFE_KM_PP_SPLIT_MIN = 8 owned undecided cubes; the cubes-only sweep of a
table below 8 192 cubes does not split: it measured slower with it, profiles/pp_split/), so the three
counters are equal to the model's attempt by attempt, and each case also asserts the property it is
there for (split ran and the remainder ran; no split in the cubes-only sweep; ties present; several
undecided trials in a split cube; the extreme cubes split; batches at the threshold).

The crafted images (zero noise, so the colours are exactly the image's) are on the cells path, where
the split runs: `rods` holds the batches at the threshold and the full ones, `corners` holds the exact ties, the cubes with several undecided trials and the
cubes at origin 0 / 252 (two sparse 64^3 regions in opposite corners of the colour space rather
than two small dense blocks: a table needs 8 192 cubes to take the cells path), `extremes` the
one-colour cubes with only bit 0 or only bit 63 set.  `ties` (two mirrored dense blocks and the
gradient sheet) stays as a cubes-only case.
"""
import numpy as np
import pytest

from low_level_feature_extraction_amd import synth
from tools import km_pp_gain_sim as sim

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

K = 5
CELL_MIN = 8192  # kmeans.hip LLFE_KM_CELL_MIN
SPLIT_MIN = 8    # kmeans.hip LLFE_KM_PP_SPLIT_MIN
SEEDS = (2027, 31)
COL_PP_PTS, COL_PP_SPLIT_CUBES, COL_PP_SPLIT_PTS = 11, 23, 24  # LLFE_KM_TRACE columns (llfe_pipeline.cpp)


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


def _gradient(side):
    y, x = np.mgrid[0:side, 0:side]
    rgb = np.stack([x * 255 // (side - 1), y * 255 // (side - 1), (x + y) * 255 // (2 * (side - 1))], -1)
    return np.ascontiguousarray(rgb[:, :, ::-1].astype(np.uint8))


def _image_of(rgb, side):
    """The colours `rgb` (n x 3, n <= side^2) as a side x side BGR image, padded with its first colour."""
    rgb = np.asarray(rgb, np.int64)
    assert len(rgb) <= side * side and rgb.min() >= 0 and rgb.max() <= 255, (len(rgb), side)
    full = np.concatenate([rgb, np.repeat(rgb[:1], side * side - len(rgb), 0)])
    return np.ascontiguousarray(full[:, ::-1].reshape(side, side, 3).astype(np.uint8))


def _block(origin, edge):
    ax = np.arange(edge)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin)


def _ties():
    """Two identical full 16^3 blocks mirrored about the plane r = 127.5 and the gradient sheet: inside a
    full block the colours equidistant from a chosen centre and a trial of the same block (both
    lattice points) fill whole planes, so G = 0 on many colours of the split cubes."""
    g = _gradient(128)[:, :, ::-1].reshape(-1, 3).astype(np.int64)
    return _image_of(np.concatenate([_block((40, 96, 96), 16), _block((200, 96, 96), 16), g]), 160)


def _corners():
    """Two 64^3 regions in opposite corners of the colour space, mirror images of each other, 4 096
    cubes each (8 192: the cells path): a cube holds its origin colour and origin + (3, 3, 3) (bits 0
    and 63), the cubes along the three edges through the corner are full.  With five centres to place in
    two regions the later rounds' trials fall beside a centre, so the bisectors cut cubes at origin 0
    and at origin 252 on every axis, full ones among them, several trials are undecided in one cube,
    and colours equidistant from a centre and a trial (all on the lattice 4a + {0, 3}) are common."""
    ax = np.arange(16) * 4
    o = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    edge = (o == 0).sum(1) >= 2
    a = np.concatenate([_block(x, 4) for x in o[edge]] + [o[~edge], o[~edge] + 3])
    return _image_of(np.concatenate([a, 255 - a]), 149)


def _rods():
    """Two rods along the red axis, 256 x 32 x 32 colours each (8 x 8 cubes per red quarter: one 64-cube
    batch of 16 whole cells; 8 192 cubes in all), every cube's origin colour and a twelfth of the rest
    present.  A centre and a trial of one rod differ mostly in red, so their bisector is nearly
    perpendicular to the red axis and cuts every cube of a red quarter at once: batches of exactly 64
    owned undecided cubes, beside the sparse ones (7, 8) where a tilted bisector leaves the rod."""
    rs = np.random.RandomState(5)
    blk = np.stack(np.meshgrid(np.arange(256), np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 3)
    corner = ((blk & 3) == 0).all(1)
    out = []
    for o in (32, 192):
        rest = blk[~corner][rs.permutation(int((~corner).sum()))[: len(blk) // 12]]
        out.append(np.concatenate([blk[corner], rest]) + np.array([0, o, o]))
    return _image_of(np.concatenate(out), 228)


def _extremes():
    """A lattice of one-colour cubes, every second cube per axis: alternately only bit 0 (the cube's
    origin colour), only bit 63 (origin + (3, 3, 3)) and one other colour, between full 8^3 blocks in
    the 8 corners.  The bisectors of far-apart centres and trials (the largest |f|) cut the lattice."""
    pts = [_block((x, y, z), 8) for x in (0, 248) for y in (0, 248) for z in (0, 248)]
    ax = np.arange(1, 31) * 8
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    kind = (lat // 8).sum(1) % 3
    off = np.where(kind[:, None] == 0, 0, np.where(kind[:, None] == 1, 3, np.array([[1, 2, 0]])))
    return _image_of(np.concatenate(pts + [lat + off]), 180)


# name -> (image, production noise (False: zero noise, the colours are exactly the image's), cells path)
CASES = {
    # cells path
    "photo160": (lambda: synth.synth_numpy(1, 160, 160, seed=2025), True, True),
    "photo256": (lambda: synth.synth_numpy(1, 256, 256, seed=2025), True, True),
    "blobs_cells": (lambda: _blobs(64, 4, 384), True, True),
    "extremes": (_extremes, False, True),
    "corners": (_corners, False, True),
    "rods": (_rods, False, True),
    # cubes-only path: no split there, every undecided cube goes one by one as before
    "photo64": (lambda: synth.synth_numpy(1, 64, 64, seed=2025), True, False),
    "blobs_cubes": (lambda: _blobs(24, 1, 176), True, False),
    "gradient256": (lambda: _gradient(256), True, False),
    "ui160": (lambda: synth.synth_numpy(0, 160, 160, seed=2025), True, False),
    "ties": (_ties, False, False),
}


def _read_trace(path):
    return np.atleast_2d(np.loadtxt(path, dtype=np.int64))


@pytest.fixture(scope="module")
def images():
    return {name: make() for name, (make, _, _) in CASES.items()}


@pytest.fixture(scope="module")
def runs(orc, images):
    """name, seed -> (noise or None, unique keys, the oracle's attempts, the model's attempts); computed once"""
    out = {}
    for name, host in images.items():
        h, w = host.shape[:2]
        for seed in SEEDS:
            noise = None if CASES[name][1] else np.zeros((h * w, 3), np.int8)
            keys = orc.color_unique(host, orc.device_noise(h * w, seed, 0) if noise is None else noise)
            st = orc.image_rng_state(seed, 0)
            out[name, seed] = (noise, keys, orc.kmeans_attempts(keys, K, st, exact_sums=True), sim.attempts_split(keys, K, st, 10, SPLIT_MIN))
    return out


def _model_sum(model, key):
    vals = [m[key] for _, m in model]
    return sum(vals[1:], vals[0])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", list(CASES))
def test_attempts_equal_exact_sum_oracle(backend, images, runs, tmp_path, monkeypatch, name, seed):
    host = images[name]
    noise, keys, ex, model = runs[name, seed]
    trace = tmp_path / "km_trace.txt"
    monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
    r = backend.process(host[None], ("colors",), seed=seed, index_base=0, noise=noise)[0]
    att = backend.kmeans_attempts(1)[0]
    assert r.n_unique == len(keys)
    n_cubes = len(np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63)))
    t = _read_trace(trace)
    assert t.shape[0] == 10 and t.shape[1] > COL_PP_SPLIT_PTS, t.shape
    dev = [int(t[:, c].sum()) for c in (COL_PP_PTS, COL_PP_SPLIT_CUBES, COL_PP_SPLIT_PTS)]
    mod = [_model_sum(model, k) for k in ("pts", "split_cubes", "split_pts")]
    print(f"{name} seed {seed}: U={len(keys)} cubes={n_cubes} device one by one / split cubes / split colours {dev}, model {mod},"
          f" one by one without the split {_model_sum(model, 'pts_before')}")
    assert (n_cubes >= CELL_MIN) == CASES[name][2], (name, n_cubes)
    for a in range(10):
        assert np.array_equal(model[a][0], ex["pp"][a].astype(np.int64)), ("model's k-means++", a)
        assert np.array_equal(att[a]["pp_centers"][:K], ex["pp"][a]), (a, att[a]["pp_centers"], ex["pp"][a])
        assert att[a]["iters"] == int(ex["iters"][a]), (a, att[a]["iters"], ex["iters"][a])
        assert np.array_equal(att[a]["centers"][:K], ex["att_centers"][a]), a
        assert np.array_equal(att[a]["counts"][:K], ex["att_counts"][a]), a
        assert abs(att[a]["compactness"] - ex["att_compactness"][a]) <= 1e-6 * ex["att_compactness"][a], a
    # the counters are what the model's batches give, attempt by attempt
    for a in range(10):
        m = model[a][1]
        assert [int(t[a, COL_PP_PTS]), int(t[a, COL_PP_SPLIT_CUBES]), int(t[a, COL_PP_SPLIT_PTS])] == \
            [m["pts"], m["split_cubes"], m["split_pts"]], (name, a)
    if CASES[name][2]:  # cells path: the split ran, and the unowned remainder still went one by one
        assert mod[1] > 0 and mod[2] > 0 and mod[0] > 0, (name, mod)
        assert dev[1] > 0 and dev[2] > 0 and dev[0] > 0, (name, dev)
    else:  # cubes-only sweep: it does not split
        assert mod[1] == 0 and mod[2] == 0 and dev[1] == 0 and dev[2] == 0 and dev[0] > 0, (name, mod, dev)


def _keys_rgb(keys):
    keys = np.asarray(keys, np.int64)
    return np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1)


def test_model_ties_in_split_cubes(runs):
    """`corners` puts colours with D = d(., t) exactly (G = 0 in a cube its nearest centre owns) into cubes
    the model splits, over every round of both seeds."""
    ties = 0
    for seed in SEEDS:
        _, keys, _, _ = runs["corners", seed]
        p = _keys_rgb(keys)
        tab = sim.CubeTable(p)
        cube_of = np.searchsorted(tab.okey, ((p[:, 0] >> 2) << 12) | ((p[:, 1] >> 3) << 7) | ((p[:, 2] >> 3) << 2) |
                                  (((p[:, 1] >> 2) & 1) << 1) | ((p[:, 2] >> 2) & 1))
        from oracle import oracle as orc
        for ch, rounds in sim.attempt_rounds(keys, K, orc.image_rng_state(seed, 0)):
            for c, tr in rounds:
                r = sim.split_round(tab, c, tr, SPLIT_MIN)
                if not r["split_idx"]:
                    continue
                sel = np.isin(cube_of, np.array(r["split_idx"]))
                q = p[sel]
                D = ((q[:, None, :] - c[None]) ** 2).sum(-1).min(1)
                for tt in tr:
                    ties += int((((q - tt) ** 2).sum(1) == D).sum())
    print(f"corners: colours of split cubes with D = d(., t) exactly: {ties}")
    assert ties >= 100, ties


def test_model_several_undecided_trials_in_a_split_cube(runs):
    """`corners` and the photos have split cubes with two and with three undecided trials: the repeated pass."""
    for name in ("corners", "photo160"):
        u = sum(_model_sum(runs[name, seed][3], "und_split") for seed in SEEDS)
        print(f"{name}: split cubes by undecided trials 1/2/3: {u[1]}/{u[2]}/{u[3]}")
        assert u[2] >= 1 and u[3] >= 1, (name, u)


def test_model_extreme_cubes_are_split(runs):
    """`corners` and `extremes`: among the cubes the model splits are cubes at origin 0 and at 252 on each
    axis, full cubes, one-colour cubes with only bit 0 and with only bit 63."""
    from oracle import oracle as orc
    seen = {"origin0": [0, 0, 0], "origin252": [0, 0, 0], "full": 0, "bit0": 0, "bit63": 0}
    for name, seed in [(n, s) for n in ("corners", "extremes") for s in SEEDS]:
        _, keys, _, _ = runs[name, seed]
        p = _keys_rgb(keys)
        tab = sim.CubeTable(p)
        cube_of = np.searchsorted(tab.okey, ((p[:, 0] >> 2) << 12) | ((p[:, 1] >> 3) << 7) | ((p[:, 2] >> 3) << 2) |
                                  (((p[:, 1] >> 2) & 1) << 1) | ((p[:, 2] >> 2) & 1))
        first = np.full(len(tab.n), -1)
        first[cube_of[::-1]] = np.arange(len(p))[::-1]  # a cube's first colour
        u = p[first] - tab.o
        bit = u[:, 0] * 16 + u[:, 1] * 4 + u[:, 2]
        idx = set()
        for ch, rounds in sim.attempt_rounds(keys, K, orc.image_rng_state(seed, 0)):
            for c, tr in rounds:
                idx.update(sim.split_round(tab, c, tr, SPLIT_MIN)["split_idx"])
        idx = np.array(sorted(idx), np.int64)
        o, n = tab.o[idx], tab.n[idx]
        for d in range(3):
            seen["origin0"][d] += int((o[:, d] == 0).sum())
            seen["origin252"][d] += int((o[:, d] == 252).sum())
        seen["full"] += int((n == 64).sum())
        seen["bit0"] += int(((n == 1) & (bit[idx] == 0)).sum())
        seen["bit63"] += int(((n == 1) & (bit[idx] == 63)).sum())
    print("extremes: split cubes by kind", seen)
    assert min(seen["origin0"] + seen["origin252"] + [seen["full"], seen["bit0"], seen["bit63"]]) > 0, seen


def test_model_batches_at_the_threshold(runs):
    """`rods`, either seed: batches with exactly SPLIT_MIN - 1 owned undecided cubes (not split), exactly
    SPLIT_MIN (split) and 64 (every lane)."""
    for seed in SEEDS:
        h = np.bincount(np.array(_model_sum(runs["rods", seed][3], "dens")), minlength=65)
        print(f"rods seed {seed}: owned undecided cubes per batch: {SPLIT_MIN - 1}: {h[SPLIT_MIN - 1]} batches, {SPLIT_MIN}: {h[SPLIT_MIN]}, 64: {h[64]}")
        assert h[SPLIT_MIN - 1] > 0 and h[SPLIT_MIN] > 0 and h[64] > 0, (seed, h)


def test_both_build_widths_split_and_agree(backend, tmp_path, monkeypatch):
    """8 photos of 160 x 160 (cells path) as a batch of 8 (80 attempts: the 512-thread build) and as the
    first 8 of a batch of 104 (1 040 attempts: the 256-thread build), same indices and seed: both
    launches split, every attempt's fields and k-means++ counters are equal."""
    big = np.stack([synth.synth_numpy(2 * i + 1, 160, 160, seed=2025) for i in range(104)])
    runs_ = []
    for tag, batch in (("wide", big[:8]), ("narrow", big)):
        trace = tmp_path / f"km_trace_{tag}.txt"
        monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
        res = backend.process(batch, ("colors",), seed=77, index_base=0)[:8]
        att = backend.kmeans_attempts(len(batch))[:8]
        t = _read_trace(trace)
        assert t.shape[0] == 10 * len(batch), (tag, t.shape)
        t = t[:80]
        n_split = int(t[:, COL_PP_SPLIT_CUBES].sum())
        print(f"{tag}: k-means++ split cubes {n_split}, their colours {int(t[:, COL_PP_SPLIT_PTS].sum())}, one by one {int(t[:, COL_PP_PTS].sum())}")
        assert n_split > 0 and int(t[:, COL_PP_SPLIT_PTS].sum()) > 0, tag
        runs_.append((res, att, t[:, [COL_PP_PTS, COL_PP_SPLIT_CUBES, COL_PP_SPLIT_PTS]]))
    (ra, aa, ta), (rb, ab, tb) = runs_
    assert np.array_equal(ta, tb)
    for i in range(8):
        assert ra[i].n_unique == rb[i].n_unique, i
        assert np.array_equal(np.asarray(ra[i].centers_rgb), np.asarray(rb[i].centers_rgb)), i
        assert np.array_equal(np.asarray(ra[i].counts), np.asarray(rb[i].counts)), i
        assert ra[i].compactness == rb[i].compactness, i
        for a in range(10):
            for f in ("pp_centers", "centers", "counts"):
                assert np.array_equal(aa[i][a][f], ab[i][a][f]), (i, a, f)
            assert aa[i][a]["iters"] == ab[i][a]["iters"] and aa[i][a]["compactness"] == ab[i][a]["compactness"], (i, a)
