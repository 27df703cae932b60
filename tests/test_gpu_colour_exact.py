"""Exact parity of the colour path (unique.hip, kmeans.hip, kmeans_big.hip) with the oracle at
small shapes: keys one by one, k-means attempt by attempt.

The cases are those of tests/colour_cases.py; tests/test_colour_exact_inputs.py shows on the CPU
that each reaches the path it is named for and that OpenCV's float32 cluster sums are exact at
these sizes, so nothing here goes through the tolerant bar of tests/kmeans_bar.py: a wrong trial
choice, tie rule or prefix walk is a failure, not "another optimum".

  A  keys and n_unique of the production noise field (no caller noise) at the 16-pixel chunk,
     the 1024-pixel wave span and the 4096-pixel step seams, three images per call, two index
     bases and two seeds; saturated images clip at 0 and 255; caller noise over all of int8,
     from a 16-byte-aligned pointer and from one a byte further on
  B  all 10 attempts for K = 2 .. 5 through process(): cube and cell sweeps, three images of
     mixed kinds per launch at index_base 1000, and the final record (k_kmeans_finalize)
  C  all 10 attempts of the plain sweeps (llfe_kmeans on caller keys): three lists of
     different lengths per call at index_base 500, lengths at the 256-point step, the 4-key lane
     and the wave-range seams, with and without the key the kernel pads with
     (B and C also on "lattice" colours, channels below 32: colours at exactly the same distance
     from two centres, which only the first-minimum rule of the labelling orders)
  D  k_kmeans_big (K = 6, 8, 32): all 10 attempts (llfe_kmeans_attempts_k) and the final record
     as a multiset, through both entry points
  E  llfe_submit_images on separately allocated device tensors, read in place and gathered
"""
import ctypes as C

import numpy as np
import pytest

from low_level_feature_extraction_amd import _lib as L
from tests import colour_cases as cc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def _dev_keys(backend, images, seed, base, noise=None):
    # (a copy: the shared case images are read-only, which torch.from_numpy warns about)
    keys, nu = backend.color_unique(np.array(images), seed=seed, noise=noise, index_base=base)
    return keys.cpu().numpy().view(np.uint32), nu


# ------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("base", cc.A_BASES)
@pytest.mark.parametrize("seed", cc.A_SEEDS)
@pytest.mark.parametrize("h,w,kind", cc.A_BATCHES)
def test_a_production_keys(backend, h, w, kind, seed, base):
    x = cc.a_images(h, w, kind)
    keys, nu = _dev_keys(backend, x, seed, base)
    for i, exp in enumerate(cc.production_keys(h, w, kind, seed, base)):
        assert nu[i] == len(exp), (i, int(nu[i]), len(exp))
        assert np.array_equal(keys[i, : nu[i]], exp), i


def _unique_with_device_noise(backend, x, noise_dev):
    """llfe_color_unique with the caller noise at the device pointer of `noise_dev` as it is
    (Backend.color_unique copies host noise into a fresh, aligned allocation)."""
    import torch

    n, h, w, _ = x.shape
    keys = torch.empty((n, h * w), dtype=torch.int32, device=x.device)
    nu = np.zeros(n, np.int64)
    b = L.LlfeBatch(C.c_void_p(x.data_ptr()), n, h, w, 1, C.c_void_p(noise_dev.data_ptr()), 1, 0, 0)
    backend._call("llfe_color_unique", C.byref(b), C.c_uint64(0), keys.data_ptr(), nu.ctypes.data, backend._stream(x))
    return keys.cpu().numpy().view(np.uint32), nu


@pytest.mark.parametrize("offset", (0, 1))
@pytest.mark.parametrize("h,w", cc.A_SHAPES)
def test_a_caller_noise_full_range(backend, orc, h, w, offset):
    import torch

    x = cc.a_images(h, w, "saturated")
    noise = cc.a_full_noise(h, w)
    xd = torch.from_numpy(np.array(x)).cuda()
    buf = torch.zeros(noise.size + 16, dtype=torch.int8, device=xd.device)
    assert buf.data_ptr() % 16 == 0
    nd = buf[offset: offset + noise.size]
    nd.copy_(torch.from_numpy(noise.reshape(-1)))
    assert nd.data_ptr() % 16 == offset
    keys, nu = _unique_with_device_noise(backend, xd, nd)
    for i in range(len(x)):
        exp = cc.numpy_unique_keys(x[i], noise[i])
        assert np.array_equal(exp, orc.color_unique(x[i], noise[i]))
        assert nu[i] == len(exp), (i, int(nu[i]), len(exp))
        assert np.array_equal(keys[i, : nu[i]], exp), i


# ------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("K", cc.B_KS)
@pytest.mark.parametrize("seed", cc.B_SEEDS)
@pytest.mark.parametrize("h,w,kind", cc.B_BATCHES)
def test_b_attempts_in_batches(backend, h, w, kind, seed, K):
    x = cc.b_images(h, w, kind)
    res = backend.process(x, ("colors",), seed=seed, index_base=cc.B_BASE, n_colors=K)
    att = backend.kmeans_attempts(3)
    keys = cc.b_keys(h, w, kind, seed)
    for i, ex in enumerate(cc.b_expected(h, w, kind, seed, K)):
        assert res[i].n_unique == len(keys[i]), i
        cc.attempts_equal(att[i], ex, K)
        cc.final_is_best_attempt(res[i].centers_rgb, res[i].counts, att[i], K)


# ------------------------------------------------------------------------------------- C
def _kmeans_on_keys(backend, key_lists, K, seed, base):
    import torch

    keys = torch.from_numpy(cc.key_buffer(key_lists).view(np.int32)).cuda()
    return backend.kmeans(keys, np.array([len(k) for k in key_lists]), K, seed=seed, index_base=base)


@pytest.mark.parametrize("K,g,kind", cc.C_CALLS)
def test_c_plain_sweep_attempts(backend, K, g, kind):
    lists = cc.c_keys(K, g, kind)
    got = _kmeans_on_keys(backend, lists, K, cc.C_SEED, cc.C_BASE)
    att = backend.kmeans_attempts(len(lists))  # (llfe_kmeans leaves its attempt records too)
    for i, ex in enumerate(cc.c_expected(K, g, kind)):
        cc.attempts_equal(att[i], ex, K)
        cc.final_is_best_attempt(got[i][0], got[i][1], att[i], K)


# ------------------------------------------------------------------------------------- D
def _final_in(centers, counts, ex, K):
    assert len(centers) == K
    assert int(np.sum(counts)) == len(ex["labels"])
    got = cc.record_multiset(centers, counts)
    ok = cc.accepted_records(ex)
    assert got in ok, (got, ok)


@pytest.mark.parametrize("K,N", cc.D_PROCESS)
def test_d_big_k_process(backend, K, N):
    seed = cc.d_process_seed(K, N)
    x = cc.d_images(N)
    res = backend.process(x, ("colors",), seed=seed, index_base=cc.D_BASE, n_colors=K)
    att = backend.kmeans_attempts(len(x), k=K)
    keys = cc.d_process_keys(N, seed)
    for i, ex in enumerate(cc.d_process_expected(K, N, seed)):
        assert res[i].n_unique == len(keys[i]), i
        _final_in(res[i].centers_rgb, res[i].counts, ex, K)
        cc.attempts_equal(att[i], ex, K)
        cc.final_is_best_attempt(res[i].centers_rgb, res[i].counts, att[i], K)


@pytest.mark.parametrize("K,g", cc.D_KEYS)
def test_d_big_k_caller_keys(backend, K, g):
    seed = cc.d_keys_seed(K, g)
    got = _kmeans_on_keys(backend, cc.d_caller_keys(K, g), K, seed, cc.D_BASE)
    att = backend.kmeans_attempts(len(got), k=K)
    for i, ex in enumerate(cc.d_keys_expected(K, g, seed)):
        _final_in(got[i][0], got[i][1], ex, K)
        cc.attempts_equal(att[i], ex, K)
        cc.final_is_best_attempt(got[i][0], got[i][1], att[i], K)


# ------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("aligned", (True, False))
@pytest.mark.parametrize("h,w", cc.E_SHAPES)
def test_e_image_tables(backend, h, w, aligned):
    """Four separately allocated device images under their own global indices: all 16-byte
    aligned and packed (read in place through the address table), or one of them a view a byte
    into its allocation (the batch is gathered first)."""
    import torch

    x = cc.e_images(h, w)
    imgs = []
    for i in range(len(x)):
        buf = torch.zeros(h * w * 3 + 16, dtype=torch.uint8, device="cuda")
        off = 1 if (not aligned and i == 1) else 0
        t = buf[off: off + h * w * 3].view(h, w, 3)
        t.copy_(torch.from_numpy(np.array(x[i])))
        assert t.data_ptr() % 16 == off and t.is_contiguous()
        imgs.append(t)
    ticket = backend.submit_images(imgs, ("colors",), seed=cc.E_SEED, indices=cc.E_INDICES, n_colors=cc.E_K)
    res = backend.collect(ticket)
    att = backend.kmeans_attempts(len(x))  # (nothing in flight any more: the ticket's workspace)
    keys = cc.e_keys(h, w)
    for i, ex in enumerate(cc.e_expected(h, w)):
        assert res[i].n_unique == len(keys[i]), i
        cc.attempts_equal(att[i], ex, cc.E_K)
        cc.final_is_best_attempt(res[i].centers_rgb, res[i].counts, att[i], cc.E_K)
        b = int(np.argmin(ex["att_compactness"]))
        assert np.array_equal(res[i].centers_rgb, ex["att_centers"][b].astype(np.uint8)), i
        assert np.array_equal(res[i].counts, ex["att_counts"][b]), i
        assert abs(res[i].compactness - ex["att_compactness"][b]) <= 1e-6 * ex["att_compactness"][b], i
