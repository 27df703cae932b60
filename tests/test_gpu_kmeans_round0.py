"""k-means++ first round in closed form, and the Lloyd iteration end (kmeans.hip).

The first k-means++ round no longer walks the cube tables: per red-quarter partition P it takes
sum_P |p - c0|^2 = Q_P - 2 c0 . S_P + n_P |c0|^2 from the partition's moments n_P, S_P = sum p,
Q_P = sum |p|^2, which k_uq_gather (unique.hip) writes once per image; sum |p|^2 of the closed-form
compactness is the sum of Q_P.  The round-0 sums decide round 1's draw and its partition prefix,
so a wrong moment shows in `pp_centers`; the sum of Q_P shows in the compactness.  The end of a
Lloyd iteration (final reduction, centre update, convergence test) runs on the lanes of one wave.

Every case runs the device on one small image and compares all 10 attempts with the oracle's
cv2.kmeans restatement in its exact-sum mode: the k-means++ centres, the Lloyd iterations, the
float32 centres and the counts are equal, the compactness within 1e-6 relative.  The images are
the smallest that reach what can go wrong here:

  red0      red channel 0 everywhere: after noise and clipping r <= 2, so every key lies in
            partition 0 and the other 63 moments are empty
  red_ends  red in {0, 255} only: partitions 0 and 63, the extreme cell origins
  photo160  >= 8 192 cubes: the sweeps of rounds >= 1 take cells / super-cells
  ui64      the cube path
  flat4     four flat, well separated colours: Lloyd ends within a few iterations (asserted on
            the oracle), so the iteration end is most of the work

The last test runs eight 64 x 64 images of the same kinds through both builds of kmeans.hip
(512-thread workgroups for launches whose attempts all fit the GPU at once, 256-thread ones
otherwise).
"""
import numpy as np
import pytest

from low_level_feature_extraction_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

K = 5
CELL_MIN = 8192  # kmeans.hip LLFE_KM_CELL_MIN
SEEDS = (2027, 31)
FLAT_SEEDS = (2027, 2)  # (seeds at which every attempt of the oracle ends within 4 iterations)


def _bgr(r, g, b):
    return np.ascontiguousarray(np.stack([b, g, r], -1).astype(np.uint8))


def _red0(side, seed=7):
    rs = np.random.RandomState(seed)
    g, b = rs.randint(0, 256, (2, side, side))
    return _bgr(np.zeros_like(g), g, b)


def _red_ends(side, seed=11):
    rs = np.random.RandomState(seed)
    g, b = rs.randint(0, 256, (2, side, side))
    return _bgr(rs.randint(0, 2, (side, side)) * 255, g, b)


def _flat4(side, seed=3):
    cols = np.array([[20, 30, 200], [220, 40, 50], [60, 210, 70], [128, 128, 128]])
    lab = np.random.RandomState(seed).randint(0, 4, (side, side))
    rgb = cols[lab]
    return _bgr(rgb[..., 0], rgb[..., 1], rgb[..., 2])


# name -> (image, partitions its keys must occupy or None, least cube count)
CASES = {
    "red0": (lambda: _red0(96), {0}, 0),
    "red_ends": (lambda: _red_ends(96), {0, 63}, 0),
    "photo160": (lambda: synth.synth_numpy(1, 160, 160, seed=2025), None, CELL_MIN),
    "ui64": (lambda: synth.synth_numpy(0, 64, 64, seed=2025), None, 0),
    "flat4": (lambda: _flat4(64), None, 0),
}


@pytest.fixture(scope="module")
def images():
    return {name: make() for name, (make, _, _) in CASES.items()}


def _n_cubes(keys):
    return len(np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63)))


@pytest.mark.parametrize("name,seed", [(n, s) for n in CASES for s in (FLAT_SEEDS if n == "flat4" else SEEDS)])
def test_attempts_equal_exact_sum_oracle(backend, orc, images, name, seed):
    host = images[name]
    h, w = host.shape[:2]
    r = backend.process(host[None], ("colors",), seed=seed, index_base=0)[0]
    att = backend.kmeans_attempts(1)[0]
    keys = orc.color_unique(host, orc.device_noise(h * w, seed, 0))
    assert r.n_unique == len(keys)
    _, parts, min_cubes = CASES[name]
    n_cubes = _n_cubes(keys)
    print(f"{name} seed {seed}: U={len(keys)} cubes={n_cubes} partitions={sorted(set((keys >> 18).tolist()))[:8]}")
    if parts is not None:
        assert set((keys >> 18).tolist()) == parts, name
    assert n_cubes >= min_cubes, (name, n_cubes)
    ex = orc.kmeans_attempts(keys, K, orc.image_rng_state(seed, 0), exact_sums=True)
    if name == "flat4":
        assert int(np.max(ex["iters"])) <= 4, ex["iters"]
    for a in range(10):
        assert np.array_equal(att[a]["pp_centers"][:K], ex["pp"][a]), (a, att[a]["pp_centers"], ex["pp"][a])
        assert att[a]["iters"] == int(ex["iters"][a]), (a, att[a]["iters"], ex["iters"][a])
        assert np.array_equal(att[a]["centers"][:K], ex["att_centers"][a]), a
        assert np.array_equal(att[a]["counts"][:K], ex["att_counts"][a]), a
        assert abs(att[a]["compactness"] - ex["att_compactness"][a]) <= 1e-6 * ex["att_compactness"][a], a


def test_both_build_widths_agree(backend):
    """Eight 64 x 64 images of the kinds above as a batch of 8 (80 attempts: the 512-thread build)
    and as the first 8 of a batch of 104 (1 040 attempts: the 256-thread build), same indices
    and seed."""
    first = [_red0(64), _red_ends(64), synth.synth_numpy(1, 64, 64, seed=2025), synth.synth_numpy(0, 64, 64, seed=2025),
             _flat4(64), _red0(64, seed=8), _red_ends(64, seed=12), _flat4(64, seed=4)]
    big = np.stack(first + [synth.synth_numpy(i, 64, 64, seed=2025) for i in range(8, 104)])
    wide = backend.process(big[:8], ("colors",), seed=77, index_base=0)
    narrow = backend.process(big, ("colors",), seed=77, index_base=0)[:8]
    for i, (a, b) in enumerate(zip(wide, narrow)):
        assert a.n_unique == b.n_unique, i
        assert np.array_equal(np.asarray(a.centers_rgb), np.asarray(b.centers_rgb)), i
        assert np.array_equal(np.asarray(a.counts), np.asarray(b.counts)), i
        assert a.compactness == b.compactness, i
