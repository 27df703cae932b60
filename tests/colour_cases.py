"""Cases and helpers of the exact colour-path tests (unique.hip, kmeans.hip, kmeans_big.hip).

tests/test_colour_exact_inputs.py checks, on the CPU, that every case reaches the path it is
named for and that exact equality with the oracle is owed; tests/test_gpu_colour_exact.py runs
the device on the same cases.  Both import the lists below, so a case cannot be edited in one
file only.  Expected values are computed once per case and shared (``functools.lru_cache``):
callers must not modify what these helpers return.

Sections (the letters are the ones the tests use):

  A  keys of the production noise (and of caller noise) at the seams of k_uq_noise / k_uq_scatter
  B  every k-means attempt for K <= 5 through process(): cube and cell tables, batches of three
  C  every attempt of the plain-sweep path (llfe_kmeans on caller keys)
  D  k_kmeans_big (K > 5): every attempt and the final record, through process() and llfe_kmeans
  E  image tables (llfe_submit_images), read in place and gathered

What each row reaches (path: field / caller = k_uq_noise + k_uq_scatter with the noise field /
with caller noise; plain, cube, cell = k_kmeans; big = k_kmeans_big; table = img_tab):

  row  shape or N                      K        path    index_base  n  seam
  A    1x1, 1x15, 1x16, 1x17, 5x7      -        field   0, 977      3  one chunk; field rounded to 16; code 62
  A    31x33, 32x32, 25x41             -        field   0, 977      3  P = 1023, 1024, 1025: the wave span
  A    63x65, 64x64, 17x241            -        field   0, 977      3  P = 4095, 4096, 4097: the scatter step
  A    3x2731, 127x129                 -        field   0, 977      3  two steps + 1, four steps - 1; wrap inside
  A    25x41, 63x65, 17x241 saturated  -        field   0, 977      3  clip at 0 and 255, partial last chunk
  A    3x2731, 127x129 red <= 1        -        field   0, 977      3  run-table entries with count 4096
  A    all 13 shapes, saturated        -        caller  0           3  int8 noise -128 .. 127, pointer % 16 = 0, 1
  B    61x67, 100x37 synth             2 .. 5   cube    1000        3  K < 5 (unused centres), LPT order, part_hist
  B    160x161 synth                   2 .. 5   cube +  1000        3  photo >= 8192 cubes beside two ui images
                                                cell
  B    61x67 lattice                   2 .. 5   cube    1000        3  exact distance ties; boxes at 0 and 255
  C    K, K + 1, 6                     2, 5     plain   500         3  N = K, one spare point, a partial lane
  C    255, 256, 257                   2, 5     plain   500         3  the 256-point wave step
  C    1023, 1025, 4097, 20001         2, 5     plain   500         3  wave ranges; key stride > N for two lists
  C    each length x with0 / without0 / quarter / lattice              the padding key as a colour; one
                                                                       partition; exact distance ties
  D    1xN, N = K, K + 1, 200, 256,    6, 8,    big     300         2  process(): contiguous keys from k_uq_gather
       257, 2049; 120x200 ui (~13 k)   32
  D    the same lengths, in pairs      6, 8,    big     300         2  llfe_kmeans: stride > N, two lengths
                                       32
  E    61x67, 64x64, aligned           5        table   2000, 2005, 4  read in place through img_tab; own indices
                                                        2001, 2009
  E    61x67, 64x64, one image + 1 B   5        gather  (the same)  4  k_gather_images, then the packed batch
"""
from __future__ import annotations

import functools

import numpy as np

from low_level_feature_extraction_amd import synth

CELL_MIN = 8192  # kmeans.hip LLFE_KM_CELL_MIN: cube count from which the sweeps take cells
ATTEMPTS = 10
IMG_SEED = 2025  # synth images


def bgr(r, g, b):
    return np.ascontiguousarray(np.stack([b, g, r], -1).astype(np.uint8))


def n_cubes(keys):
    """Occupied 4 x 4 x 4 cubes of the colour space."""
    keys = np.asarray(keys, np.uint32)
    return len(np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63)))


def rgb_of(keys):
    keys = np.asarray(keys, np.uint32)
    return np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], -1)


def _orc():
    from oracle import oracle

    oracle.lib()
    return oracle


# ------------------------------------------------------------------------------------- A
# (h, w): P = 1, 15, 16, 17 (the 16-pixel chunk and the field's rounding to 16), 35, then one
# below / at / one above the 1024-pixel wave span and the 4096-pixel scatter step, two steps
# plus one pixel, and four steps less one
A_SHAPES = ((1, 1), (1, 15), (1, 16), (1, 17), (5, 7), (31, 33), (32, 32), (25, 41), (63, 65), (64, 64), (17, 241),
            (3, 2731), (127, 129))
A_SEEDS = (2027, 31)
A_BASES = (0, 977)
A_N = 3
A_SATURATED = ((25, 41), (63, 65), (17, 241))  # also all-0, all-255 and a 0 / 255 checker
A_RED = ((3, 2731), (127, 129))               # also red <= 1: every key in partition 0
A_BATCHES = tuple([(h, w, "natural") for h, w in A_SHAPES] + [(h, w, "saturated") for h, w in A_SATURATED] +
                  [(h, w, "red") for h, w in A_RED])


def _natural(h, w, n=A_N):
    """Random pixels below 32 px on a side, synth images (ui, photo, ui, ...) above."""
    if h >= 32 and w >= 32:
        return np.stack([synth.synth_numpy(i, h, w, seed=IMG_SEED) for i in range(n)])
    rng = np.random.default_rng(h * 100003 + w)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _saturated(h, w):
    y, x = np.mgrid[0:h, 0:w]
    chk = np.repeat((((x + y) & 1) * 255)[..., None], 3, -1).astype(np.uint8)
    return np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), chk])


def _red01(h, w, seed):
    rs = np.random.RandomState(seed)
    r, g, b = rs.randint(0, 2, (h, w)), rs.randint(0, 256, (h, w)), rs.randint(0, 256, (h, w))
    return bgr(r, g, b)


@functools.lru_cache(maxsize=None)
def a_images(h, w, kind):
    """The three BGR images of one call of A."""
    if kind == "natural":
        x = _natural(h, w)
    elif kind == "saturated":
        x = _saturated(h, w)
    else:  # two images with red <= 1 (after noise red <= 3: partition 0 only) and a natural one
        x = np.stack([_red01(h, w, 1), _red01(h, w, 2), _natural(h, w, 1)[0]])
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def a_full_noise(h, w, n=A_N):
    """Caller noise over all of int8 for a batch of n h x w images (RGB order)."""
    rs = np.random.RandomState(h * 7919 + w)
    return rs.randint(-128, 128, (n, h * w, 3)).astype(np.int8)


def numpy_unique_keys(img_bgr, noise):
    """np.unique of clip(rgb + noise, 0, 255), packed r << 16 | g << 8 | b."""
    rgb = img_bgr.reshape(-1, 3)[:, ::-1].astype(np.int64)
    v = np.clip(rgb + np.asarray(noise, np.int64).reshape(-1, 3), 0, 255)
    return np.unique(v[:, 0] << 16 | v[:, 1] << 8 | v[:, 2]).astype(np.uint32)


def field_rotation(P, seed, a, b):
    """By how many pixels image index b reads the (seed, P) noise field further on than index a:
    the rotation search of test_oracle_device_noise.py (at P = L every field pixel is read
    once, so the two noises are rotations of one another by a multiple of 16).  -> the
    rotations that fit (one, unless the field repeats itself)."""
    O = _orc()
    L = (max(P, 1) + 15) // 16 * 16
    fa, fb = O.device_noise(L, seed, a), O.device_noise(L, seed, b)
    return [s for s in range(0, L, 16) if np.array_equal(np.roll(fa, -s, axis=0), fb)]


@functools.lru_cache(maxsize=None)
def production_keys(h, w, kind, seed, base):
    """Oracle keys of each image of an A batch under the production noise."""
    O = _orc()
    x = a_images(h, w, kind)
    return tuple(O.color_unique(x[i], O.device_noise(h * w, seed, base + i)) for i in range(len(x)))


# ------------------------------------------------------------------------------------- B
B_SHAPES = ((61, 67), (100, 37), (160, 161))
# "synth": ui, photo, ui.  "lattice": random colours inside a box 24 wide at the bottom, the
# middle and the top of the colour space -- small integer coordinates, so many colours lie at
# exactly the same distance from two k-means++ centres (which are colours themselves) and the
# first-minimum rule of the labelling decides
B_BATCHES = tuple([(h, w, "synth") for h, w in B_SHAPES] + [(61, 67, "lattice")])
B_KS = (2, 3, 4, 5)
B_SEEDS = (2027, 31)
B_BASE = 1000
B_CELL_IMAGE = (160, 161, "synth", 1)  # the photo that must reach the cell path


@functools.lru_cache(maxsize=None)
def b_images(h, w, kind):
    if kind == "synth":
        x = np.stack([synth.synth_numpy(i, h, w, seed=IMG_SEED) for i in range(3)])
    else:
        rs = np.random.RandomState(h * w)
        x = np.stack([rs.randint(lo, lo + 24, (h, w, 3)).astype(np.uint8) for lo in (0, 116, 232)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def b_keys(h, w, kind, seed):
    O = _orc()
    x = b_images(h, w, kind)
    return tuple(O.color_unique(x[i], O.device_noise(h * w, seed, B_BASE + i)) for i in range(3))


@functools.lru_cache(maxsize=None)
def b_expected(h, w, kind, seed, K, exact_sums=True):
    O = _orc()
    return tuple(O.kmeans_attempts(k, K, O.image_rng_state(seed, B_BASE + i), exact_sums=exact_sums)
                 for i, k in enumerate(b_keys(h, w, kind, seed)))


def first_labelling_ties(keys, ex):
    """How many (colour, attempt) pairs have the colour at exactly the same float32 distance
    from its two nearest k-means++ centres: ties in the first labelling of the attempts."""
    p = rgb_of(keys).astype(np.float32)
    ties = 0
    for a in range(ATTEMPTS):
        d = ((p[:, None, :] - np.asarray(ex["pp"][a], np.float32)[None, :, :]) ** 2).sum(-1)  # (integers: exact)
        d.sort(axis=1)
        ties += int((d[:, 0] == d[:, 1]).sum())
    return ties


# ------------------------------------------------------------------------------------- C
C_KS = (2, 5)
C_SEED = 77
C_BASE = 500
# "lattice": colours with every channel below 32, for exact distance ties (see B_BATCHES)
C_KINDS = ("with0", "without0", "quarter", "lattice")
C_QUARTER = 37  # the partition (key >> 18: four values of red) of the "quarter" sets


def c_lengths(K):
    """Ten lengths -- K and K + 1 points, 6, the 256-point wave step, the 4-key lane tail and the
    wave ranges of the sweeps -- as four calls of three lists of different lengths (two
    lengths come twice, with different keys)."""
    return ((K, 256, 1025), (K + 1, 257, 4097), (6, 255, 1023), (20001, K, 257))


C_CALLS = tuple((K, g, kind) for K in C_KS for g in range(4) for kind in C_KINDS)


def random_keys(N, kind, salt):
    """N sorted unique keys: with key 0x000000 (the value the kernels pad with), without it,
    inside partition C_QUARTER only, or on the lattice of channels below 32 (without key 0)."""
    rs = np.random.RandomState(salt)
    if kind == "lattice":
        cells = rs.permutation(32 ** 3 - 1)[:N] + 1
        keys = (cells >> 10) << 16 | (cells >> 5 & 31) << 8 | (cells & 31)
    elif kind == "quarter":
        pool = np.unique(rs.randint(0, 1 << 18, 3 * N + 16))
        keys = pool[rs.permutation(len(pool))[:N]] + (C_QUARTER << 18)
    else:
        pool = np.unique(rs.randint(1, 1 << 24, 2 * N + 16))
        keys = pool[rs.permutation(len(pool))[:N]]
        if kind == "with0":
            keys[0] = 0
    keys = np.unique(keys).astype(np.uint32)
    assert len(keys) == N
    return keys


@functools.lru_cache(maxsize=None)
def c_keys(K, g, kind):
    out = tuple(random_keys(N, kind, 1000 * K + 10 * g + j) for j, N in enumerate(c_lengths(K)[g]))
    for k in out:
        k.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def c_expected(K, g, kind, exact_sums=True):
    O = _orc()
    return tuple(O.kmeans_attempts(k, K, O.image_rng_state(C_SEED, C_BASE + i), exact_sums=exact_sums)
                 for i, k in enumerate(c_keys(K, g, kind)))


def key_buffer(key_lists):
    """(n, stride) uint32 buffer of the lists, zero padded, stride a multiple of 4."""
    stride = max(4, (max(len(k) for k in key_lists) + 3) // 4 * 4)
    buf = np.zeros((len(key_lists), stride), np.uint32)
    for i, k in enumerate(key_lists):
        buf[i, : len(k)] = k
    return buf


# ------------------------------------------------------------------------------------- D
D_KS = (6, 8, 32)
D_BASE = 300
D_UI_SHAPE = (120, 200)  # about 13 k unique colours
NEAR_TIE = 1e-6          # the device's compactness differs from the oracle's by ~1e-7 relative
CLEAR_GAP = 1e-4


def d_lengths(K):
    return (K, K + 1, 200, 256, 257, 2049)


# process(): two images per call -- "grid": 1 x N pixels of distinct colours 5 apart in every
# channel, which |noise| <= 2 keeps distinct, so U = N; "ui": the 120 x 200 ui images.
# llfe_kmeans: two key lists of different lengths per call ("ui": the oracle keys of D_UI_SHAPE)
D_PROCESS = tuple((K, N) for K in D_KS for N in d_lengths(K) + ("ui",))


def d_key_pairs(K):
    return ((K, 2049), (K + 1, 257), (200, 256), ("ui", K + 1))


D_KEYS = tuple((K, g) for K in D_KS for g in range(4))

# Seeds per case: the first of 1, 2, 3, ... at which no image of the case has a near-tie between
# the oracle's attempts (test_colour_exact_inputs.py asserts it).  Uniformly random colours in
# 8 clusters have many optima about 1e-5 apart, hence the two late seeds.
D_PROCESS_SEEDS = {(6, 257): 2, (8, 2049): 46}  # (K, N) -> seed; every other case: 1
D_KEYS_SEEDS = {(6, 0): 5, (6, 2): 3, (8, 0): 152}  # (K, call) -> seed; every other case: 1


def d_process_seed(K, N):
    return D_PROCESS_SEEDS.get((K, N), 1)


def d_keys_seed(K, g):
    return D_KEYS_SEEDS.get((K, g), 1)


@functools.lru_cache(maxsize=None)
def d_images(N):
    if N == "ui":
        x = np.stack([synth.synth_numpy(2 * i, *D_UI_SHAPE, seed=IMG_SEED) for i in range(2)])
    else:
        rs = np.random.RandomState(40000 + N)
        out = []
        for _ in range(2):
            cells = rs.permutation(51 ** 3)[:N]
            rgb = np.stack([cells // 2601, cells // 51 % 51, cells % 51], -1) * 5 + 2
            out.append(bgr(rgb[:, 0], rgb[:, 1], rgb[:, 2]).reshape(1, N, 3))
        x = np.stack(out)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def d_process_keys(N, seed):
    O = _orc()
    x = d_images(N)
    P = x.shape[1] * x.shape[2]
    return tuple(O.color_unique(x[i], O.device_noise(P, seed, D_BASE + i)) for i in range(2))


@functools.lru_cache(maxsize=None)
def d_process_expected(K, N, seed, exact_sums=True):
    O = _orc()
    return tuple(O.kmeans_attempts(k, K, O.image_rng_state(seed, D_BASE + i), exact_sums=exact_sums)
                 for i, k in enumerate(d_process_keys(N, seed)))


@functools.lru_cache(maxsize=None)
def d_caller_keys(K, g):
    out = []
    for j, N in enumerate(d_key_pairs(K)[g]):
        if N == "ui":
            O = _orc()
            img = d_images("ui")[0]
            out.append(O.color_unique(img, O.numpy_noise(img.shape[0] * img.shape[1], 5)))
        else:
            out.append(random_keys(N, "without0", 7000 + 100 * K + 10 * g + j))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def d_keys_expected(K, g, seed, exact_sums=True):
    O = _orc()
    return tuple(O.kmeans_attempts(k, K, O.image_rng_state(seed, D_BASE + i), exact_sums=exact_sums)
                 for i, k in enumerate(d_caller_keys(K, g)))


def record_multiset(centers, counts):
    """Sorted list of (r, g, b, count): a final record without its centre order."""
    c = np.asarray(centers).reshape(-1, 3)
    return sorted((int(c[k, 0]), int(c[k, 1]), int(c[k, 2]), int(counts[k])) for k in range(len(c)))


def attempt_record(ex, a):
    """Attempt a of an oracle result as a final record: centers.astype(uint8) and the counts."""
    return record_multiset(ex["att_centers"][a].astype(np.uint8), ex["att_counts"][a])


def best_gap(ex):
    """(best attempt, relative distance from its compactness to the next different one or inf,
    whether the attempts tied with the best give the same record)."""
    comp = np.asarray(ex["att_compactness"], np.float64)
    best = int(np.argmin(comp))  # the first of the smallest
    above = comp[comp > comp[best]]
    gap = float("inf") if len(above) == 0 or comp[best] == 0 else float((above.min() - comp[best]) / comp[best])
    rec = attempt_record(ex, best)
    same = all(attempt_record(ex, a) == rec for a in range(len(comp)) if comp[a] == comp[best])
    return best, gap, same


def accepted_records(ex):
    """The final records a device may give for an oracle result: the best attempt's, and the
    runner-up's where the two compactnesses are unequal but within NEAR_TIE relative (float
    rounding of the device's compactness may then order them either way)."""
    comp = np.asarray(ex["att_compactness"], np.float64)
    order = np.argsort(comp, kind="stable")
    out = [attempt_record(ex, int(order[0]))]
    c0, c1 = comp[order[0]], comp[order[1]]
    if c0 != c1 and c1 - c0 <= NEAR_TIE * c0:
        out.append(attempt_record(ex, int(order[1])))
    return out


# ------------------------------------------------------------------------------------- E
E_SHAPES = ((61, 67), (64, 64))
E_SEED = 2027
E_INDICES = (2000, 2005, 2001, 2009)
E_K = 5


@functools.lru_cache(maxsize=None)
def e_images(h, w):
    x = np.stack([synth.synth_numpy(i, h, w, seed=IMG_SEED + 1) for i in range(4)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def e_keys(h, w):
    O = _orc()
    x = e_images(h, w)
    return tuple(O.color_unique(x[i], O.device_noise(h * w, E_SEED, g)) for i, g in enumerate(E_INDICES))


@functools.lru_cache(maxsize=None)
def e_expected(h, w, exact_sums=True):
    O = _orc()
    return tuple(O.kmeans_attempts(k, E_K, O.image_rng_state(E_SEED, g), exact_sums=exact_sums)
                 for k, g in zip(e_keys(h, w), E_INDICES))


# ------------------------------------------------------------------------------- comparisons
def attempts_equal(got, ex, K):
    """Assert that the device's attempt records `got` (Backend.kmeans_attempts, one image; 5
    rows, or k rows with k > 5) equal the oracle's `ex`: k-means++ centres, Lloyd iterations,
    float32 centres and counts exactly, compactness within 1e-6 relative; centres and counts
    past row K are zero."""
    assert len(got) == ATTEMPTS
    for a in range(ATTEMPTS):
        g = got[a]
        assert len(g["centers"]) >= K and not np.any(g["centers"][K:]) and not np.any(g["counts"][K:]), ("rows", a)
        assert np.array_equal(g["pp_centers"][:K], ex["pp"][a]), ("pp", a, g["pp_centers"][:K], ex["pp"][a])
        assert g["iters"] == int(ex["iters"][a]), ("iters", a, g["iters"], int(ex["iters"][a]))
        assert np.array_equal(g["centers"][:K], ex["att_centers"][a]), ("centers", a, g["centers"][:K],
                                                                          ex["att_centers"][a])
        assert np.array_equal(g["counts"][:K], ex["att_counts"][a]), ("counts", a, g["counts"][:K],
                                                                        ex["att_counts"][a])
        want = float(ex["att_compactness"][a])
        assert abs(g["compactness"] - want) <= 1e-6 * want, ("compactness", a, g["compactness"], want)


def final_is_best_attempt(centers_rgb, counts, got, K):
    """Assert that a final record is the device's own best attempt (k_kmeans_finalize): the
    first attempt with the smallest compactness, its first K centres truncated to uint8."""
    assert len(np.asarray(centers_rgb).reshape(-1, 3)) == K == len(counts)
    comp = [g["compactness"] for g in got]
    b = comp.index(min(comp))
    assert np.array_equal(np.asarray(centers_rgb), got[b]["centers"][:K].astype(np.uint8)), (b, centers_rgb)
    assert np.array_equal(np.asarray(counts), got[b]["counts"][:K]), (b, counts)


def same_attempts(x, y):
    """Whether two oracle results (exact_sums False / True) hold identical attempts."""
    return all(np.array_equal(x[f], y[f]) for f in ("pp", "iters", "att_centers", "att_counts", "att_compactness"))
