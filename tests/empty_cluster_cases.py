"""Key sets on which an attempt of cv2.kmeans moves a point into an empty cluster.

OpenCV gives a cluster that lost all its points the farthest point of the biggest cluster
(kmeans.cpp; oracle/llfe_oracle.c orc_kmeans_ex).  The device restates that rule three times --
k_kmeans on plain keys, k_kmeans on cube tables with segmented keys, k_kmeans_big -- each with
its own farthest-point reduction (the larger index wins on equal distance), its list of moved
points (moved_label) and, on cube tables, the closed-form compactness from the adjusted sums.
No case of tests/colour_cases.py reaches the rule (tests/test_empty_cluster_inputs.py asserts it
for sections B, C and D), so the cases below are the only coverage.  They come from
tools/find_empty_cluster_cases.py: about one (key set, seed) pair in 10^5 moves a point, nearly
always in an attempt that does not win, which is why the tests compare every attempt.

tests/test_empty_cluster_inputs.py checks the table on the CPU oracle;
tests/test_gpu_kmeans_empty_cluster.py runs the device.  The cv::RNG state of a case is
image_rng_state(seed, index) with seed + index = s (it depends on the sum only).

  case      K   N   s           moves in attempt  winner  from
  rand4a    4   23  271060668   6                 3       the issue that asked for these tests (uniform)
  line4b    4   14  741758565   9                 0       tool: line, K=4
  line4c    4   11  17509823    3                 0       tool: line, K=4
  gray5a    5   27  862556438   2                 4       tool: line (d = 1: grays), K=5
  line5b    5   23  390810721   6                 2       tool: line, K=5
  win5a     5   18  500532180   0                 0       tool: line, K=5; the moving attempt wins
  win5b     5   12  126092587   0                 0       tool: line (grays), K=5; the moving attempt wins
  line6     6   19  996902449   8                 0       tool: line, K=6
  win6      6   18  371704362   4                 4       tool: line (grays), K=6; the moving attempt wins
  line8     8   35  915902572   7                 1       the issue
  line32a   32  99  749777563   8                 9       the issue
  line32b   32  77  707609088   1                 6       tool: line, K=32
  gray32c   32  124 1056697545  3                 9       tool: line (d = 1: grays), K=32

Every case moves one point in one Lloyd update of one attempt, with a single farthest point.
In win5a, win5b and win6 the moving attempt wins, so the final record itself carries the moved
point.  Also searched for, and not found in the 2.3 x 10^7 (key set, seed) pairs the tool was
given (1.8 x 10^7 with K = 2 .. 5, 4.5 x 10^6 with K = 6 and 8, 4 x 10^5 with K = 32, 8 x 10^4
of them with N in 300 .. 700): an attempt with two moves in one update, a move decided among
equally far points, and a case with N > 256.  All 21 hits of the tool came from the near-one-dimensional
generator; the uniform, lattice and large-N generators gave none.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import colour_cases as cc

BASE = 700        # index_base of every device call; the case's seed is s - BASE
AGAIN = 2         # the case's keys again at index BASE + AGAIN, where no attempt moves a point
WIDE_BATCH = 104  # images from which k_kmeans runs in its 256-thread build (1 040 attempts)


def _hex(text):
    return tuple(int(t, 16) for t in text.split())


def _line(rs, d):
    return tuple(r << 16 | (r // d) << 8 | (r // d) for r in rs)


_R32A = (2, 5, 6, 7, 10, 13, 14, 18, 19, 23, 27, 28, 30, 31, 34, 35, 38, 39, 42, 46, 47, 49, 52, 54, 61, 63, 66, 68, 73,
         77, 79, 80, 84, 89, 91, 95, 96, 98, 102, 103, 104, 106, 108, 109, 110, 115, 117, 122, 123, 124, 135, 139, 146,
         147, 148, 151, 152, 154, 155, 164, 165, 169, 170, 172, 177, 178, 185, 186, 187, 190, 194, 197, 199, 200, 201,
         204, 207, 210, 211, 214, 217, 221, 222, 224, 230, 231, 232, 234, 235, 237, 243, 244, 245, 248, 250, 251, 253,
         254, 255)

_R32B = (4, 6, 7, 10, 14, 17, 20, 21, 24, 26, 27, 30, 31, 32, 35, 36, 37, 38, 44, 46, 49, 52, 57, 62, 63, 66,
         68, 70, 74, 80, 82, 93, 95, 98, 102, 103, 106, 107, 108, 110, 111, 119, 126, 132, 133, 134, 144, 149,
         155, 161, 162, 164, 166, 172, 181, 183, 185, 188, 189, 190, 191, 198, 212, 214, 219, 220, 224, 225,
         227, 234, 240, 241, 243, 245, 248, 249, 254)
_R32C = (0, 3, 6, 7, 8, 18, 22, 23, 24, 25, 28, 31, 32, 34, 36, 39, 40, 41, 43, 45, 48, 49, 52, 53, 54, 55,
         56, 57, 60, 61, 63, 66, 69, 71, 75, 76, 78, 82, 83, 84, 93, 94, 95, 96, 97, 98, 100, 101, 108, 109,
         113, 114, 118, 119, 120, 121, 122, 128, 130, 131, 134, 135, 137, 139, 141, 142, 143, 148, 150, 154,
         155, 156, 157, 162, 163, 164, 165, 168, 177, 180, 181, 182, 183, 186, 187, 188, 189, 190, 191, 195,
         196, 198, 199, 202, 203, 207, 208, 209, 210, 211, 212, 214, 218, 219, 222, 224, 227, 228, 229, 236,
         237, 238, 242, 243, 244, 245, 246, 247, 248, 249, 250, 252, 253, 255)

# name -> (K, s, moving attempt, winner, keys in np.unique order)
CASES = {
    "rand4a": (4, 271060668, 6, 3, _hex(
        "0e60b9 17563c 1dc28b 2f776b 313e2a 42cece 47707f 578b99 5f8711 677b4b 6ea551 7964f4 84656b 865528 8ed08d "
        "94c377 99d741 9c9022 c1c3a4 c4a227 eae7f1 f2aada fcaf94")),
    "line4b": (4, 741758565, 9, 0, _hex(
        "140606 351111 371212 4b1919 7d2929 7f2a2a 872d2d be3f3f c44141 ca4343 d84848 da4848 dc4949 ea4e4e")),
    "line4c": (4, 17509823, 3, 0, _hex(
        "050202 1f0f0f 321919 763b3b 914848 9f4f4f cd6666 d06868 d46a6a d86c6c e37171")),
    "gray5a": (5, 862556438, 2, 4, _hex(
        "101010 171717 1b1b1b 202020 2e2e2e 323232 4a4a4a 505050 545454 5a5a5a 5e5e5e 676767 686868 707070 8c8c8c "
        "979797 a4a4a4 afafaf b0b0b0 b4b4b4 b5b5b5 dadada dcdcdc e8e8e8 eaeaea ededed fdfdfd")),
    "line5b": (5, 390810721, 6, 2, _hex(
        "090404 0d0606 0f0707 130909 140a0a 2d1616 3e1f1f 492424 542a2a 5b2d2d 603030 613030 643232 6a3535 6c3636 "
        "6d3636 8a4545 8d4646 9c4e4e c06060 c66363 c86464 e77373")),
    "win5a": (5, 500532180, 0, 0, _hex(
        "200a0a 250c0c 270d0d 2a0e0e 421616 471717 5b1e1e 5f1f1f 672222 682222 8d2f2f 9a3333 9b3333 a23636 d44646 "
        "e84d4d f15050 f95353")),
    "win5b": (5, 126092587, 0, 0, _hex("171717 191919 222222 696969 747474 757575 7b7b7b 9e9e9e a2a2a2 a5a5a5 c6c6c6 eeeeee")),
    "line6": (6, 996902449, 8, 0, _hex(
        "070101 0b0202 0c0303 1e0707 2f0b0b 581616 671919 691a1a 6a1a1a 7a1e1e 7f1f1f 802020 812020 872121 9d2727 "
        "a12828 ab2a2a d03434 e13838")),
    "line8": (8, 915902572, 7, 1, _hex(
        "000000 0a0202 0c0303 120404 140505 170505 190606 300c0c 340d0d 360d0d 421010 461111 4a1212 4f1313 521414 "
        "581616 651919 771d1d 842121 9c2727 a42929 ac2b2b b82e2e ba2e2e c13030 c93232 cb3232 d13434 d63535 db3636 "
        "dc3737 e73939 ea3a3a ef3b3b fd3f3f")),
    "win6": (6, 371704362, 4, 4, _hex(
        "030303 0c0c0c 151515 161616 202020 212121 323232 5e5e5e 606060 6f6f6f 848484 858585 878787 999999 c2c2c2 "
        "c5c5c5 cecece efefef")),
    "line32a": (32, 749777563, 8, 9, _line(_R32A, 3)),
    "line32b": (32, 707609088, 1, 6, _line(_R32B, 4)),
    "gray32c": (32, 1056697545, 3, 9, _line(_R32C, 1)),
}
NAMES = tuple(CASES)
SMALL_K = tuple(n for n in NAMES if CASES[n][0] <= 5)  # k_kmeans; the others k_kmeans_big


def case_keys(name):
    keys = np.array(CASES[name][4], np.uint32)
    keys.setflags(write=False)
    return keys


def case_seed(name):
    return CASES[name][1] - BASE


@functools.lru_cache(maxsize=None)
def key_lists(name):
    """The three lists of one llfe_kmeans call: the case (index BASE), a list 7 keys longer
    (BASE + 1), and the case again (BASE + AGAIN)."""
    keys = case_keys(name)
    other = cc.random_keys(len(keys) + 7, "without0", 9000 + NAMES.index(name))
    other.setflags(write=False)
    return keys, other, keys


@functools.lru_cache(maxsize=None)
def images(name, n=3):
    """n BGR images of 1 x N pixels: the case's colours, N other colours, the case again, and
    (n > 3: the batch that takes the 256-thread build) further random colours."""
    keys = case_keys(name)
    N = len(keys)
    lists = [keys, cc.random_keys(N, "without0", 9100 + NAMES.index(name)), keys]
    lists += [cc.random_keys(N, "without0", 9200 + 200 * NAMES.index(name) + i) for i in range(3, n)]
    rgb = np.stack([cc.rgb_of(k) for k in lists])
    x = np.ascontiguousarray(rgb[:, None, :, ::-1].astype(np.uint8))
    x.setflags(write=False)
    return x


def image_keys(name):
    """The key lists of the first three images(name): with zero noise, their colours."""
    keys = case_keys(name)
    return keys, cc.random_keys(len(keys), "without0", 9100 + NAMES.index(name)), keys


def _expected(name, lists, exact_sums):
    O = cc._orc()
    K, seed = CASES[name][0], case_seed(name)
    return tuple(O.kmeans_attempts(k, K, O.image_rng_state(seed, BASE + i), exact_sums=exact_sums)
                 for i, k in enumerate(lists))


@functools.lru_cache(maxsize=None)
def keys_expected(name, exact_sums=True):
    return _expected(name, key_lists(name), exact_sums)


@functools.lru_cache(maxsize=None)
def images_expected(name, exact_sums=True):
    return _expected(name, image_keys(name), exact_sums)
