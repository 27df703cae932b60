"""k-means++ on gains (kmeans.hip pp_cubes): each round accumulates g_j = sum max(0, D - d(., t_j))
per trial and takes T_j = sum(D) - g_j, instead of summing T_j itself.  A box far from the three
trials is decided (gain 0) even where a bisector between two chosen centres cuts it, so the
decision paths differ from the sums' -- the totals, and so every choice, may not.

Every case runs the device on one small image and compares all 10 attempts with the oracle's
cv2.kmeans restatement in its exact-sum mode (orc_kmeans_ex): the k-means++ centres, the Lloyd
iterations, the float32 centres and the counts are equal, the compactness within 1e-6 relative.
The images are the smallest that reach each path of the sweep (cube count against the 8 192
threshold from which the sweeps take cells / super-cells; the cube count is recomputed here
from the oracle's unique colours, 4 x 4 x 4 cubes of the colour space).

The last test runs the same images through both builds of kmeans.hip (512-thread workgroups
for launches whose attempts all fit the GPU at once, 256-thread ones otherwise).
"""
import numpy as np
import pytest

from low_level_feature_extraction_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

K = 5
CELL_MIN = 8192  # kmeans.hip LLFE_KM_CELL_MIN
SEEDS = (2027, 31)


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


# name -> (image, cube-count range asserted: which path the sweeps take)
CASES = {
    "photo160": (lambda: synth.synth_numpy(1, 160, 160, seed=2025), (CELL_MIN, 1 << 18)),  # cells / super-cells
    "photo256": (lambda: synth.synth_numpy(1, 256, 256, seed=2025), (CELL_MIN, 1 << 18)),  # denser boxes
    "photo64": (lambda: synth.synth_numpy(1, 64, 64, seed=2025), (1024, CELL_MIN - 1)),    # cubes only
    "ui160": (lambda: synth.synth_numpy(0, 160, 160, seed=2025), (64, 4096)),              # many empty partitions
    "blobs_cubes": (lambda: _blobs(24, 1, 176), (256, CELL_MIN - 1)),
    "blobs_cells": (lambda: _blobs(64, 4, 384), (CELL_MIN, 1 << 18)),
    "gradient256": (lambda: _gradient(256), (4096, CELL_MIN - 1)),  # a dense sheet across several bisectors
}


@pytest.fixture(scope="module")
def images():
    return {name: make() for name, (make, _) in CASES.items()}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", list(CASES))
def test_attempts_equal_exact_sum_oracle(backend, orc, images, name, seed):
    host = images[name]
    h, w = host.shape[:2]
    r = backend.process(host[None], ("colors",), seed=seed, index_base=0)[0]
    att = backend.kmeans_attempts(1)[0]
    keys = orc.color_unique(host, orc.device_noise(h * w, seed, 0))
    assert r.n_unique == len(keys)
    n_cubes = len(np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63)))
    lo, hi = CASES[name][1]
    print(f"{name} seed {seed}: U={len(keys)} cubes={n_cubes}")
    assert lo <= n_cubes <= hi, (name, n_cubes)
    ex = orc.kmeans_attempts(keys, K, orc.image_rng_state(seed, 0), exact_sums=True)
    for a in range(10):
        assert np.array_equal(att[a]["pp_centers"][:K], ex["pp"][a]), (a, att[a]["pp_centers"], ex["pp"][a])
        assert att[a]["iters"] == int(ex["iters"][a]), (a, att[a]["iters"], ex["iters"][a])
        assert np.array_equal(att[a]["centers"][:K], ex["att_centers"][a]), a
        assert np.array_equal(att[a]["counts"][:K], ex["att_counts"][a]), a
        assert abs(att[a]["compactness"] - ex["att_compactness"][a]) <= 1e-6 * ex["att_compactness"][a], a


def test_both_build_widths_agree(backend):
    """8 images of 64 x 64 as a batch of 8 (80 attempts: the 512-thread build) and as the first
    8 of a batch of 104 (1 040 attempts: the 256-thread build), same indices and seed."""
    big = np.stack([synth.synth_numpy(i, 64, 64, seed=2025) for i in range(104)])
    wide = backend.process(big[:8], ("colors",), seed=77, index_base=0)
    narrow = backend.process(big, ("colors",), seed=77, index_base=0)[:8]
    for i, (a, b) in enumerate(zip(wide, narrow)):
        assert a.n_unique == b.n_unique, i
        assert np.array_equal(np.asarray(a.centers_rgb), np.asarray(b.centers_rgb)), i
        assert np.array_equal(np.asarray(a.counts), np.asarray(b.counts)), i
        assert a.compactness == b.compactness, i
