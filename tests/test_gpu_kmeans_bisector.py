"""Lloyd's bisector split of two-centre boundary cubes (kmeans.hip bisector_signs): a cube that fails
the margin test against exactly one other centre j is split in place by the sign of
F = d_j - d_k, walked in fixed point over its 64 positions; only the colours with |F| <= 0.5 are
still labelled one by one.  A colour the split puts on the wrong side of a bisector changes a
count or a centre, so every case compares all 10 attempts of one small image with the oracle's
cv2.kmeans restatement in its exact-sum mode (OpenCV's float labelling): k-means++ centres,
iterations, float32 centres and counts equal, compactness within 1e-6 relative.

The LLFE_KM_TRACE line of each attempt carries the cubes split in place and the colours they
decided; the tests read them to see that the split ran where the batches are dense (cells path),
stayed out where failures are sparse (ui: the cubes-only sweep of a small table never splits), and
that the ambiguous / multi-centre remainder still went through the one-by-one labelling.
"""
import numpy as np
import pytest

from low_level_feature_extraction_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

K = 5
CELL_MIN = 8192  # kmeans.hip LLFE_KM_CELL_MIN
SEEDS = (2027, 31)
COL_LL_PTS, COL_SPLIT_CUBES, COL_SPLIT_PTS = 15, 17, 18  # LLFE_KM_TRACE columns (llfe_pipeline.cpp)


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


# name -> (image, cells path (cube count >= CELL_MIN), split expected: True / False / None = either)
CASES = {
    "photo160": (lambda: synth.synth_numpy(1, 160, 160, seed=2025), True, True),
    "photo256": (lambda: synth.synth_numpy(1, 256, 256, seed=2025), True, True),
    "blobs_cells": (lambda: _blobs(64, 4, 384), True, True),
    "gradient256": (lambda: _gradient(256), False, None),  # a dense sheet across several bisectors (cubes only: no split)
    "ui160": (lambda: synth.synth_numpy(0, 160, 160, seed=2025), False, False),  # sparse failures: the old path
}
PHOTOS = ("photo160", "photo256")


def _read_trace(path):
    return np.atleast_2d(np.loadtxt(path, dtype=np.int64))


@pytest.fixture(scope="module")
def images():
    return {name: make() for name, (make, _, _) in CASES.items()}


@pytest.fixture(scope="module")
def oracle_runs(orc, images):
    """name, seed -> (unique keys, the oracle's attempts); computed once, read by both tests"""
    out = {}
    for name, host in images.items():
        h, w = host.shape[:2]
        for seed in SEEDS:
            keys = orc.color_unique(host, orc.device_noise(h * w, seed, 0))
            out[name, seed] = (keys, orc.kmeans_attempts(keys, K, orc.image_rng_state(seed, 0), exact_sums=True))
    return out


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", list(CASES))
def test_attempts_equal_exact_sum_oracle(backend, images, oracle_runs, tmp_path, monkeypatch, name, seed):
    host = images[name]
    trace = tmp_path / "km_trace.txt"
    monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
    r = backend.process(host[None], ("colors",), seed=seed, index_base=0)[0]
    att = backend.kmeans_attempts(1)[0]
    keys, ex = oracle_runs[name, seed]
    assert r.n_unique == len(keys)
    n_cubes = len(np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63)))
    _, cells, split = CASES[name]
    t = _read_trace(trace)
    assert t.shape[0] == 10 and t.shape[1] > COL_SPLIT_PTS, t.shape
    n_split, n_split_pts, ll_pts = int(t[:, COL_SPLIT_CUBES].sum()), int(t[:, COL_SPLIT_PTS].sum()), int(t[:, COL_LL_PTS].sum())
    print(f"{name} seed {seed}: U={len(keys)} cubes={n_cubes} split cubes={n_split} colours decided={n_split_pts} "
          f"labelled one by one={ll_pts}")
    assert (n_cubes >= CELL_MIN) == cells, (name, n_cubes)
    for a in range(10):
        assert np.array_equal(att[a]["pp_centers"][:K], ex["pp"][a]), (a, att[a]["pp_centers"], ex["pp"][a])
        assert att[a]["iters"] == int(ex["iters"][a]), (a, att[a]["iters"], ex["iters"][a])
        assert np.array_equal(att[a]["centers"][:K], ex["att_centers"][a]), a
        assert np.array_equal(att[a]["counts"][:K], ex["att_counts"][a]), a
        assert abs(att[a]["compactness"] - ex["att_compactness"][a]) <= 1e-6 * ex["att_compactness"][a], a
    if split is True:
        assert n_split > 0 and n_split_pts > 0, (name, n_split, n_split_pts)
    if split is False:
        assert n_split == 0 and n_split_pts == 0, (name, n_split, n_split_pts)
    if name in PHOTOS:
        assert ll_pts > 0, name  # the ambiguous and multi-centre remainder still ran


def _near_ties(keys, centres):
    """Over the cubes of `keys` that fail the Lloyd margin test against exactly one centre j (owner k =
    first minimum at the cube centre): the colours with d_j = d_k exactly, and with 0 < |d_j - d_k| <= 0.5
    (float64: exact for float32 centres and integer colours at these magnitudes)."""
    c = centres.astype(np.float64)
    p = np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], -1).astype(np.float64)
    cube = ((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63)
    ids, inv = np.unique(cube, return_inverse=True)
    q = np.stack([(ids >> 12) & 63, (ids >> 6) & 63, ids & 63], -1) * 4.0 + 1.5
    dq = ((q[:, None, :] - c[None]) ** 2).sum(-1)
    k = dq.argmin(1)
    thr = 3.0 * np.abs(c[None, :, :] - c[k][:, None, :]).sum(-1) + 1.0
    cont = dq - dq[np.arange(len(ids)), k][:, None] <= thr
    cont[np.arange(len(ids)), k] = False
    two = cont.sum(1) == 1
    j = cont.argmax(1)
    sel = two[inv]
    kk, jj, pp = k[inv][sel], j[inv][sel], p[sel]
    f = ((pp - c[jj]) ** 2).sum(-1) - ((pp - c[kk]) ** 2).sum(-1)
    return int((f == 0).sum()), int(((f != 0) & (np.abs(f) <= 0.5)).sum())


@pytest.mark.parametrize("name", PHOTOS)
def test_near_ties_are_present(oracle_runs, name):
    """The photo cases really put colours on and next to a bisector of their two-centre cubes
    (attempts 0-2 of seed 2027, every sweep's centres from the oracle's iter_centers)."""
    keys, ex = oracle_runs[name, 2027]
    ties = amb = 0
    for a in range(3):
        sweeps = [ex["pp"][a]] + [ex["iter_centers"][a, i] for i in range(int(ex["iters"][a]) - 1)]
        for cen in sweeps:
            if np.isnan(cen).any():
                continue
            t, m = _near_ties(keys, cen)
            ties += t
            amb += m
    print(f"{name}: U={len(keys)} exact ties {ties}, colours with 0 < |d_j - d_k| <= 0.5: {amb}")
    assert ties >= 1 and amb >= 1, (ties, amb)


def test_both_build_widths_split_and_agree(backend, tmp_path, monkeypatch):
    """104 photos of 160 x 160 as one batch (1 040 attempts: the 256-thread build) and its first 2 as a
    batch of 2 (20 attempts: the 512-thread build), same indices and seed: the split runs in both
    launches and the results are equal."""
    big = np.stack([synth.synth_numpy(2 * i + 1, 160, 160, seed=2025) for i in range(104)])
    runs = []
    for tag, batch in (("wide", big[:2]), ("narrow", big)):
        trace = tmp_path / f"km_trace_{tag}.txt"
        monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
        res = backend.process(batch, ("colors",), seed=77, index_base=0)[:2]
        t = _read_trace(trace)
        assert t.shape[0] == 10 * len(batch), (tag, t.shape)
        n_split = int(t[:, COL_SPLIT_CUBES].sum())
        print(f"{tag}: split cubes {n_split}, colours decided {int(t[:, COL_SPLIT_PTS].sum())}")
        assert n_split > 0, tag
        runs.append(res)
    for i, (a, b) in enumerate(zip(*runs)):
        assert a.n_unique == b.n_unique, i
        assert np.array_equal(np.asarray(a.centers_rgb), np.asarray(b.centers_rgb)), i
        assert np.array_equal(np.asarray(a.counts), np.asarray(b.counts)), i
        assert a.compactness == b.compactness, i
