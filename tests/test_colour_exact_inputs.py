"""Preconditions of the exact colour-path cases (tests/colour_cases.py), on the CPU oracle.

tests/test_gpu_colour_exact.py asks the device for exact equality with the oracle.  That is
owed only where the oracle's own answer does not depend on what the device legitimately does
differently, and it tests a path only if the case reaches it.  So, for every case:

* OpenCV's sequential float32 cluster sums (exact_sums=False) and the device's exact int64
  sums (exact_sums=True) give identical attempts: every cluster sum stays below 2^24 at these
  sizes (U * 255 < 2^24), so the float32 sums are exact and no attempt may differ;
* the images of B hold the cube counts that select the cube / cell sweeps;
* the shapes of A that span a wave (P >= 1024) are read at a non-zero rotation of the noise
  field by at least one tested index, so the wrap (p + o) mod L falls inside the image; the
  saturated images clip at both ends; the red <= 1 images keep every key in partition 0;
* no case of D has a near-tie between the oracle's attempts: the best attempt's compactness
  is at least 1e-4 relative below the next different one, and attempts tied with it exactly
  give the same record, so the expected final record does not hang on float rounding.
"""
import numpy as np
import pytest

from tests import colour_cases as cc


# ------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("seed", cc.A_SEEDS)
@pytest.mark.parametrize("h,w", [s for s in cc.A_SHAPES if s[0] * s[1] >= 1024])
def test_a_some_index_reads_a_rotated_field(orc, h, w, seed):
    P = h * w
    for base in cc.A_BASES:
        # the offsets of the call's later images relative to its first: one unequal to 0 means
        # that not all of them can be 0
        rel = [cc.field_rotation(P, seed, base, base + i) for i in range(1, cc.A_N)]
        assert all(len(r) == 1 for r in rel), rel
        assert any(r[0] != 0 for r in rel), (h, w, seed, base, rel)


def test_a_shapes_cover_the_seams():
    P = [h * w for h, w in cc.A_SHAPES]
    assert {1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 16383} <= set(P)
    for h, w in cc.A_SATURATED + cc.A_RED:
        assert (h, w) in cc.A_SHAPES
    assert any(p % 16 for p in (h * w for h, w in cc.A_SATURATED))  # a partial last chunk that clips


@pytest.mark.parametrize("h,w", cc.A_SATURATED)
def test_a_saturated_images_clip_at_both_ends(orc, h, w):
    x = cc.a_images(h, w, "saturated").astype(np.int64)
    for seed in cc.A_SEEDS:
        for base in cc.A_BASES:
            lo = hi = 0
            for i in range(cc.A_N):
                v = x[i].reshape(-1, 3)[:, ::-1] + orc.device_noise(h * w, seed, base + i)
                lo += int((v < 0).sum())
                hi += int((v > 255).sum())
            assert lo > 0 and hi > 0, (h, w, seed, base, lo, hi)


def test_a_caller_noise_spans_int8():
    for h, w in cc.A_SHAPES:
        nz = cc.a_full_noise(h, w)
        assert nz.dtype == np.int8 and nz.shape == (cc.A_N, h * w, 3)
        if h * w >= 1024:
            assert nz.min() == -128 and nz.max() == 127


@pytest.mark.parametrize("h,w", cc.A_RED)
def test_a_red_images_fill_one_partition(h, w):
    P = h * w
    assert P > 2 * 4096  # at least two whole 4096-key steps
    for seed in cc.A_SEEDS:
        for base in cc.A_BASES:
            keys = cc.production_keys(h, w, "red", seed, base)
            for k in keys[:2]:
                assert int(k.max()) >> 18 == 0
            assert len(set((keys[2] >> 18).tolist())) > 1  # (the third image is an ordinary one)


# ------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("seed", cc.B_SEEDS)
@pytest.mark.parametrize("h,w,kind", cc.B_BATCHES)
def test_b_cube_counts_select_the_paths(h, w, kind, seed):
    keys = cc.b_keys(h, w, kind, seed)
    cubes = [cc.n_cubes(k) for k in keys]
    print(h, w, kind, seed, [len(k) for k in keys], cubes)
    assert cubes[0] < cc.CELL_MIN and cubes[2] < cc.CELL_MIN  # the ui images: cube sweeps
    if (h, w, kind, 1) == cc.B_CELL_IMAGE:
        assert cubes[1] >= cc.CELL_MIN  # the photo: cell / super-cell sweeps
    assert all(len(k) * 255 < 1 << 24 for k in keys)


@pytest.mark.parametrize("K", cc.B_KS)
@pytest.mark.parametrize("seed", cc.B_SEEDS)
@pytest.mark.parametrize("h,w,kind", cc.B_BATCHES)
def test_b_float32_sums_are_exact(h, w, kind, seed, K):
    keys = cc.b_keys(h, w, kind, seed)
    exs = cc.b_expected(h, w, kind, seed, K)
    for f32, ex in zip(cc.b_expected(h, w, kind, seed, K, exact_sums=False), exs):
        assert cc.same_attempts(f32, ex)
    if kind == "lattice":  # every image has colours the first-minimum rule decides
        ties = [cc.first_labelling_ties(k, ex) for k, ex in zip(keys, exs)]
        assert min(ties) > 0, ties


# ------------------------------------------------------------------------------------- C
def test_c_lengths_and_key_sets():
    for K in cc.C_KS:
        flat = [N for g in cc.c_lengths(K) for N in g]
        assert {K, K + 1, 6, 255, 256, 257, 1023, 1025, 4097, 20001} == set(flat)
        for g in range(4):
            assert len(set(cc.c_lengths(K)[g])) == 3  # three different lengths: a real stride
            for kind in cc.C_KINDS:
                for keys, N in zip(cc.c_keys(K, g, kind), cc.c_lengths(K)[g]):
                    assert len(keys) == N and np.all(np.diff(keys.astype(np.int64)) > 0)
                    assert (keys[0] == 0) == (kind == "with0")
                    if kind == "quarter":
                        assert set((keys >> 18).tolist()) == {cc.C_QUARTER}
                    if kind == "lattice":
                        assert int(cc.rgb_of(keys).max()) < 32


@pytest.mark.parametrize("K,g,kind", cc.C_CALLS)
def test_c_float32_sums_are_exact(K, g, kind):
    exs = cc.c_expected(K, g, kind)
    for f32, ex in zip(cc.c_expected(K, g, kind, exact_sums=False), exs):
        assert cc.same_attempts(f32, ex)
    if kind == "lattice":  # the longer lists have colours the first-minimum rule decides
        for keys, ex in zip(cc.c_keys(K, g, kind), exs):
            if len(keys) >= 255:
                assert cc.first_labelling_ties(keys, ex) > 0, len(keys)


# ------------------------------------------------------------------------------------- D
def _clear_best(ex):
    best, gap, same = cc.best_gap(ex)
    assert same, "attempts tied with the best give different records"
    assert gap >= cc.CLEAR_GAP, gap
    assert len(cc.accepted_records(ex)) == 1  # the near-tie exemption is not needed


@pytest.mark.parametrize("K,N", cc.D_PROCESS)
def test_d_process_cases(K, N):
    seed = cc.d_process_seed(K, N)
    keys = cc.d_process_keys(N, seed)
    if N == "ui":
        assert all(10000 <= len(k) <= 30000 for k in keys), [len(k) for k in keys]
    else:
        assert all(len(k) == N for k in keys), [len(k) for k in keys]  # U = N: the noise merges no colours
    f32s, exs = cc.d_process_expected(K, N, seed, exact_sums=False), cc.d_process_expected(K, N, seed)
    for f32, ex in zip(f32s, exs):
        assert cc.same_attempts(f32, ex)
        _clear_best(ex)


@pytest.mark.parametrize("K,g", cc.D_KEYS)
def test_d_caller_key_cases(K, g):
    seed = cc.d_keys_seed(K, g)
    keys = cc.d_caller_keys(K, g)
    assert len(keys[0]) != len(keys[1]) and all(len(k) <= 30000 for k in keys)
    for f32, ex in zip(cc.d_keys_expected(K, g, seed, exact_sums=False), cc.d_keys_expected(K, g, seed)):
        assert cc.same_attempts(f32, ex)
        _clear_best(ex)


def test_d_lengths():
    for K in cc.D_KS:
        want = {K, K + 1, 200, 256, 257, 2049, "ui"}
        assert {N for k, N in cc.D_PROCESS if k == K} == want
        assert {N for g in cc.d_key_pairs(K) for N in g} == want


# ------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("h,w", cc.E_SHAPES)
def test_e_float32_sums_are_exact(h, w):
    for f32, ex in zip(cc.e_expected(h, w, exact_sums=False), cc.e_expected(h, w)):
        assert cc.same_attempts(f32, ex)
