"""The move into an empty cluster on the device, attempt by attempt (kmeans.hip, kmeans_big.hip).

A cluster that lost all its points takes the farthest point of the biggest cluster.  The cases
of tests/empty_cluster_cases.py each make one such move, nearly always in an attempt that does
not win, so every test compares all 10 attempts with the oracle (colour_cases.attempts_equal:
k-means++ centres, iterations, float32 centres and counts exactly, compactness within 1e-6
relative) and the final record with the device's own best attempt.
tests/test_empty_cluster_inputs.py shows on the CPU that each case makes its move and that exact
equality is owed.

Each case goes through every door that reaches another implementation of the rule:

  keys     llfe_kmeans on caller keys, three lists per call (the case, a longer list, the case
           again under an index that moves nothing), key stride > N: the plain sweep of k_kmeans
           for K <= 5, k_kmeans_big above
  process  llfe_process_batch on 1 x N images of exactly those colours with zero caller noise:
           k_kmeans on cube tables with segmented keys (the partition-by-partition walk, the
           closed-form compactness from the adjusted sums) for K <= 5, k_kmeans_big behind
           k_uq_gather above
  narrow   K <= 5: the same images first in a batch of 104, which takes the 256-thread build of
           kmeans.hip; its attempts equal the 512-thread build's
"""
import numpy as np
import pytest

from tests import colour_cases as cc
from tests import empty_cluster_cases as ec

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def _process(backend, name, n):
    K = ec.CASES[name][0]
    x = ec.images(name, n)
    noise = np.zeros((n, x.shape[2], 3), np.int8)
    res = backend.process(np.array(x), ("colors",), seed=ec.case_seed(name), noise=noise, index_base=ec.BASE,
                          n_colors=K)
    return res, backend.kmeans_attempts(3, k=K)


@pytest.mark.parametrize("name", ec.NAMES)
def test_caller_keys(backend, name):
    import torch

    K = ec.CASES[name][0]
    lists = ec.key_lists(name)
    buf = cc.key_buffer(lists)
    assert buf.shape[1] > len(lists[0])
    got = backend.kmeans(torch.from_numpy(buf.view(np.int32)).cuda(), np.array([len(k) for k in lists]), K,
                         seed=ec.case_seed(name), index_base=ec.BASE)
    att = backend.kmeans_attempts(len(lists), k=K)
    for i, ex in enumerate(ec.keys_expected(name)):
        cc.attempts_equal(att[i], ex, K)
        cc.final_is_best_attempt(got[i][0], got[i][1], att[i], K)


@pytest.mark.parametrize("name", ec.NAMES)
def test_process_zero_noise(backend, orc, name):
    K = ec.CASES[name][0]
    res, att = _process(backend, name, 3)
    x = ec.images(name)
    keys, nu = backend.color_unique(np.array(x), seed=ec.case_seed(name), noise=np.zeros((3, x.shape[2], 3), np.int8),
                                    index_base=ec.BASE)
    keys = keys.cpu().numpy().view(np.uint32)
    for i, (want, ex) in enumerate(zip(ec.image_keys(name), ec.images_expected(name))):
        assert res[i].n_unique == len(want) == nu[i], i
        assert np.array_equal(keys[i, : nu[i]], want), i
        cc.attempts_equal(att[i], ex, K)
        cc.final_is_best_attempt(res[i].centers_rgb, res[i].counts, att[i], K)


@pytest.mark.parametrize("name", ec.SMALL_K)
def test_narrow_build(backend, name):
    K = ec.CASES[name][0]
    _, wide = _process(backend, name, 3)
    res, narrow = _process(backend, name, ec.WIDE_BATCH)
    for i, ex in enumerate(ec.images_expected(name)):
        cc.attempts_equal(narrow[i], ex, K)
        cc.final_is_best_attempt(res[i].centers_rgb, res[i].counts, narrow[i], K)
        for a in range(cc.ATTEMPTS):
            for f in ("pp_centers", "centers", "counts"):
                assert np.array_equal(narrow[i][a][f], wide[i][a][f]), (i, a, f)
            assert narrow[i][a]["iters"] == wide[i][a]["iters"] and \
                narrow[i][a]["compactness"] == wide[i][a]["compactness"], (i, a)
