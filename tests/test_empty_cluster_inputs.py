"""Preconditions of the empty-cluster cases (tests/empty_cluster_cases.py), on the CPU oracle.

tests/test_gpu_kmeans_empty_cluster.py asks the device for all 10 attempts of every case, equal
to the oracle's.  That tests the move into an empty cluster only if the case makes one, and is
owed only where the oracle's answer does not hang on rounding.  So, for every case:

* the attempt its table row names moves a point (relocations > 0), no other attempt does, and
  the row's winner is the oracle's; the same keys at index BASE + AGAIN move nothing;
* OpenCV's float32 cluster sums and the device's exact int64 sums give identical attempts;
* no two attempts have unequal compactnesses within NEAR_TIE relative (the device's compactness
  differs from the oracle's by ~1e-7 relative, which must not reorder attempts; attempts with
  exactly equal compactness are compared one by one like the others, and the final record is
  checked against the device's own first minimum);
* through process() the K <= 5 cases run k_kmeans on cube tables with segmented keys:
  llfe_process_batch gathers contiguous keys only for n_colors > 5 (color_stage's
  contiguous_keys) and otherwise hands k_kmeans the cube tables and part_hist, so its
  empty-cluster branch walks the keys partition by partition.  What the case must add is shown
  here: fewer cubes than the cell sweeps need, and keys in more than one red-quarter partition
  (so the walk crosses segment boundaries) with the moved point's cluster among them.

Sections B, C and D of tests/colour_cases.py still reach no move: the new cases are the only
coverage of the rule.
"""
import hashlib
import subprocess
import sys

import numpy as np
import pytest

from tests import colour_cases as cc
from tests import empty_cluster_cases as ec


def _no_near_tie(ex):
    comp = np.sort(np.asarray(ex["att_compactness"], np.float64))
    gaps = np.diff(comp)
    assert not np.any((gaps > 0) & (gaps <= cc.NEAR_TIE * comp[:-1])), comp


@pytest.mark.parametrize("name", ec.NAMES)
def test_case_moves_a_point_where_its_row_says(name):
    K, s, moving, winner, keys = ec.CASES[name]
    assert list(keys) == sorted(set(keys)) and len(keys) > K  # np.unique order
    for exs in (ec.keys_expected(name), ec.images_expected(name)):
        ex = exs[0]
        print(name, K, len(keys), ex["relocations"], ex["relocations_max"], ex["relocation_ties"], ex["iters"])
        assert ex["relocations"][moving] > 0
        assert [a for a in range(cc.ATTEMPTS) if ex["relocations"][a]] == [moving]
        assert int(np.argmin(ex["att_compactness"])) == winner
        assert not np.any(exs[ec.AGAIN]["relocations"])  # the same keys under another index: no move
        assert np.all(ex["relocations_max"] <= ex["relocations"]) and np.all(ex["relocation_ties"] <= ex["relocations"])


def test_issue_cases_iterations():
    assert ec.keys_expected("rand4a")[0]["iters"].tolist() == [4, 4, 5, 3, 5, 4, 5, 4, 5, 4]
    assert ec.keys_expected("line8")[0]["iters"].tolist() == [4, 5, 3, 5, 3, 3, 4, 5, 7, 4]


@pytest.mark.parametrize("name", ec.NAMES)
def test_float32_sums_are_exact_and_no_near_tie(name):
    for f32s, exs in ((ec.keys_expected(name, False), ec.keys_expected(name)),
                      (ec.images_expected(name, False), ec.images_expected(name))):
        for f32, ex in zip(f32s, exs):
            assert cc.same_attempts(f32, ex)
            assert np.array_equal(f32["relocations"], ex["relocations"])
            _no_near_tie(ex)


def test_required_cases_are_there():
    ks = [ec.CASES[n][0] for n in ec.NAMES]
    small = [k for k in ks if k <= 5]
    assert len(small) >= 3 and len(set(small)) >= 2      # the issue's K = 4 case and two more, one not K = 4
    assert len([k for k in ks if k > 5]) >= 4 and ks.count(32) >= 2


@pytest.mark.parametrize("name", ec.NAMES)
def test_call_layouts(name):
    keys, other, again = ec.key_lists(name)
    assert len(other) != len(keys) and np.array_equal(keys, again)
    assert cc.key_buffer(ec.key_lists(name)).shape[1] > len(keys)  # a key stride greater than N
    x = ec.images(name)
    assert x.shape == (3, 1, len(keys), 3)
    for img, k in zip(x, ec.image_keys(name)):  # zero noise: the keys are the colours
        assert np.array_equal(cc._orc().color_unique(img, np.zeros((len(k), 3), np.int8)), k)


@pytest.mark.parametrize("name", ec.SMALL_K)
def test_small_k_cases_cross_segments_on_cube_tables(name):
    keys = ec.case_keys(name)
    assert cc.n_cubes(keys) < cc.CELL_MIN
    parts = keys >> 18
    assert len(set(parts.tolist())) > 1
    # the moving attempt's biggest cluster -- the one the farthest-point walk reads -- holds more
    # than one partition's keys: it has more points than the fullest partition
    K, _, moving, _, _ = ec.CASES[name]
    ex = ec.images_expected(name)[0]
    assert int(ex["att_counts"][moving].max()) + 1 > int(np.bincount(parts).max())
    assert ec.images(name, ec.WIDE_BATCH).shape[0] * cc.ATTEMPTS > 1024


def test_sections_b_c_d_move_nothing():
    def none(exs):
        return not any(np.any(ex["relocations"]) for ex in exs)

    for h, w, kind in cc.B_BATCHES:
        for seed in cc.B_SEEDS:
            for K in cc.B_KS:
                assert none(cc.b_expected(h, w, kind, seed, K)), (h, w, kind, seed, K)
    for K, g, kind in cc.C_CALLS:
        assert none(cc.c_expected(K, g, kind)), (K, g, kind)
    for K, N in cc.D_PROCESS:
        assert none(cc.d_process_expected(K, N, cc.d_process_seed(K, N))), (K, N)
    for K, g in cc.D_KEYS:
        assert none(cc.d_keys_expected(K, g, cc.d_keys_seed(K, g))), (K, g)


_DIGEST = """
import hashlib
from tests import empty_cluster_cases as ec
h = hashlib.sha256(repr(sorted(ec.CASES.items())).encode())
for n in ec.NAMES:
    for k in ec.key_lists(n):
        h.update(k.tobytes())
    h.update(ec.images(n).tobytes())
print(h.hexdigest())
"""


def test_module_is_deterministic():
    out = [subprocess.run([sys.executable, "-c", _DIGEST], capture_output=True, text=True, check=True,
                          cwd=cc.__file__.rsplit("/tests/", 1)[0]).stdout.strip() for _ in range(2)]
    h = hashlib.sha256(repr(sorted(ec.CASES.items())).encode())
    for n in ec.NAMES:
        for k in ec.key_lists(n):
            h.update(k.tobytes())
        h.update(ec.images(n).tobytes())
    assert out[0] == out[1] == h.hexdigest() and len(out[0]) == 64
