"""Class maps for the union-find hysteresis (hysteresis.hip) that no NMS output looks like.

tests/test_hysteresis_inputs.py checks, on the CPU, that every case is what its row says;
tests/test_gpu_hysteresis_classes.py runs llfe_hysteresis on the same cases.  Both import the
catalogue below, so a case cannot be edited in one file only.  Maps and expected outputs are
computed once per case and shared (``functools.lru_cache``): callers must not modify them.

A class map is a u8 array of 0 (weak), 1 (none) and 2 (strong).  The reference is plain
8-connected component labelling: a candidate (byte != 1) is kept iff its component holds a 2;
the mask is the kept set dilated 3 x 3.

What each row reaches (a tile is 64 x 64; lane = tile row; lab = the local root of a run):

  row  shapes                     cases                                  seam
  a    1x1, 1x200, 200x1, 64x64,  all 1 / all 0 / all 0 + one 2 in the   empty list; one run per row; partial
       65x65, 127x129             last pixel / all 2                     tiles of 1 row / column; 64-wide runs
  i    200x330, 192x320           p = .05 .3 .41 .6 .9, strong share     bytewise / 16-byte row reader; below, at
                                  .05 / .0005 of candidates, 2 seeds     and above percolation; promoted roots
  b    130x130                    (y + x) even -> 0; one 2 at (128,128)  32 runs per row (node ids up to 2047);
                                  / no 2                                 diagonal-only contacts; all promoted
  c    193x200                    even columns 0; a 2 in the bottom row  32 roots per tile, a third of them
                                  of every third stripe                  promoted from the last tile row up
  d    193x200, 200x193, 192x192  serpentine rows / columns, spiral;     union chains through every tile and back
                                  one 2 at the far end
  e    192x192, 130x130           diagonal, anti-diagonal (+ a weak      k_ccl_border's diagonal looks at a tile
                                  parallel 3 columns off); pixel pairs   corner, full and partial tiles beyond
                                  across the corner (64,64) / (128,128);
                                  pairs across a bottom edge mid-tile    its south-east / south-west looks alone
  f    130x200, 1x1000, 3x1000    single pixels at x = 63 / 64; a run    lab at x = 63 (lrow[63]) and at run
                                  60..66; a full row; runs ending at 63  starts; the east look of the right column
                                  in tile rows 0, 1, 62, 63
  g    130x130                    teeth on even columns joined by tile   many roots merged by lane 63 / by the
                                  row 63 / hanging from tile row 0       border pass into one global root
  h    130x130                    weak block / ring at Chebyshev         what must not be united
                                  distance 2 of a strong dot

Every case runs inside a batch of three (``batch``): an all-1 image, the case, and another
case of the same shape.
"""
from __future__ import annotations

import functools

import numpy as np

T = 64  # hysteresis tile edge


def reference(cls):
    """(edges, mask) of one class map: components of cls != 1 that hold a 2; 3 x 3 dilation."""
    from scipy import ndimage

    lab, k = ndimage.label(cls != 1, structure=np.ones((3, 3)))
    keep = np.zeros(k + 1, bool)
    keep[np.unique(lab[cls == 2])] = True
    keep[0] = False
    edges = (keep[lab] * 255).astype(np.uint8)
    mask = ndimage.maximum_filter(edges, size=3, mode="constant", cval=0)
    return edges, mask


def promoted(cls):
    """Kept pixels whose tile-local component holds no 2 (they need the global unions)."""
    edges, _ = reference(cls)
    local = np.zeros_like(edges)
    h, w = cls.shape
    for y in range(0, h, T):
        for x in range(0, w, T):
            local[y:y + T, x:x + T] = reference(cls[y:y + T, x:x + T])[0]
    return (edges == 255) & (local == 0)


def tiles_spanned(cls):
    """Largest number of tiles a kept component has pixels in."""
    from scipy import ndimage

    lab, k = ndimage.label(cls != 1, structure=np.ones((3, 3)))
    ys, xs = np.nonzero(reference(cls)[0])
    if not len(ys):
        return 0
    ntx = (cls.shape[1] + T - 1) // T
    pairs = np.unique(np.stack([lab[ys, xs], (ys // T) * ntx + xs // T], 1), axis=0)
    return int(np.bincount(pairs[:, 0]).max())


def runs_per_row(cls):
    """Largest number of candidate runs in one 64-pixel tile row."""
    c = np.pad(cls != 1, ((0, 0), (0, (-cls.shape[1]) % T)))
    c = c.reshape(c.shape[0], -1, T)
    starts = c & ~np.concatenate([np.zeros_like(c[..., :1]), c[..., :-1]], -1)
    return int(starts.sum(-1).max())


def _ones(h, w):
    return np.ones((h, w), np.uint8)


# ------------------------------------------------------------------------------------- a
A_SHAPES = ((1, 1), (1, 200), (200, 1), (64, 64), (65, 65), (127, 129))


def _trivial(kind, h, w):
    c = np.full((h, w), {"none": 1, "weak": 0, "last2": 0, "strong": 2}[kind], np.uint8)
    if kind == "last2":
        c[-1, -1] = 2
    return c


# ------------------------------------------------------------------------------------- i
I_SHAPES = ((200, 330), (192, 320))  # W % 16 != 0: the bytewise row reader; W % 16 == 0: 16-byte loads
I_P = (0.05, 0.3, 0.41, 0.6, 0.9)
I_SHARE = (0.05, 0.0005)
I_SEEDS = (11, 12)


def _random(h, w, p, share, seed):
    rng = np.random.default_rng([seed, h, w, int(p * 100), int(share * 10000)])
    cand = rng.random((h, w)) < p
    strong = cand & (rng.random((h, w)) < share)
    c = _ones(h, w)
    c[cand] = 0
    c[strong] = 2
    return c


# ------------------------------------------------------------------------------------- b - h
def _checker(with2):
    y, x = np.mgrid[:130, :130]
    c = np.where((y + x) % 2 == 0, 0, 1).astype(np.uint8)
    if with2:
        c[128, 128] = 2
    return c


def _stripes():
    c = _ones(193, 200)
    c[:, ::2] = 0
    c[192, ::6] = 2  # stripe k sits at x = 2 k: every third stripe
    return c


def _serpentine():
    h, w = 193, 200
    c = _ones(h, w)
    c[::2] = 0
    for k, y in enumerate(range(1, h, 2)):
        c[y, w - 1 if k % 2 == 0 else 0] = 0
    c[192, 199] = 2  # row 192 is entered at x = 0 (k = 95 is odd): the far end
    return c


def _spiral(n=192):
    c = _ones(n, n)
    seen = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1

    def free(yy, xx):  # a step to (yy, xx) keeps a one-pixel gap to the arm beyond it
        if not (0 <= yy < n and 0 <= xx < n) or seen[yy, xx]:
            return False
        y2, x2 = yy + dy, xx + dx
        return not (0 <= y2 < n and 0 <= x2 < n and seen[y2, x2])

    while True:
        seen[y, x] = True
        if not free(y + dy, x + dx):
            dy, dx = dx, -dy
            if not free(y + dy, x + dx):
                break
        y, x = y + dy, x + dx
    c[seen] = 0
    c[y, x] = 2  # the inner end
    return c


def _diagonal(anti, end):
    n = 192
    c = _ones(n, n)
    i = np.arange(n)
    xs = n - 1 - i if anti else i
    j = np.arange(40, 150)  # a weak parallel 3 columns off: Chebyshev distance 2, never united
    c[j, (n - 1 - j - 3) if anti else j + 3] = 0
    c[i, xs] = 0
    c[i[end], xs[end]] = 2
    return c


def _corner_pair(n, k, anti, second):
    """The two pixels that touch only through the tile corner (k, k) of an n x n map, the 2
    on the first or second; the same pair, weak only, at the other corner (dropped)."""
    c = _ones(n, n)
    pair = [(k - 1, k), (k, k - 1)] if anti else [(k - 1, k - 1), (k, k)]
    for p in pair:
        c[p] = 0
    c[pair[second]] = 2
    o = 64 if k == 128 else 128
    for p in ([(o - 1, o), (o, o - 1)] if anti else [(o - 1, o - 1), (o, o)]):
        c[p] = 0
    return c


def _south_diag():
    """Pairs that touch diagonally over a tile's bottom edge away from its corners: only the
    bottom row's south-east / south-west looks of k_ccl_border unite them (at a corner the
    right column's east looks do it as well).  Below full and partial tiles."""
    c = _ones(130, 130)
    for y in (63, 127):
        c[y, 20], c[y + 1, 21] = 2, 0
        c[y, 40], c[y + 1, 39] = 0, 2
        c[y, 100], c[y + 1, 101] = 0, 0  # weak only: dropped
    return c


F_SHAPE = (130, 200)


def _px63(y0):
    """Single-pixel runs at x = 63 and x = 64 that touch diagonally over the tile edge, from
    row y0 down: strong at 63 + weak at 64, weak at 63 + strong at 64, and one of each alone."""
    c = _ones(*F_SHAPE)
    c[y0, 63], c[y0 + 1, 64] = 2, 0
    c[y0 + 4, 64], c[y0 + 3, 63] = 2, 0
    c[y0 + 7, 63] = 0  # alone: dropped
    c[y0 + 10, 64] = 0
    return c


def _run6066(at):
    c = _ones(*F_SHAPE)
    c[20, 60:67] = 0
    c[20, at] = 2
    c[22, 60:67] = 0  # two rows off: dropped
    c[70, 124:131] = 0  # the same over the next tile edge, strong at the other end
    c[70, 190 - at] = 2
    return c


def _fullrow(h, at):
    c = _ones(h, 1000)
    c[h // 2] = 0
    c[h // 2, at] = 2
    return c


def _end63(r, tail2):
    """A run 40..63 in row r of a tile (in both tile rows of the map), met diagonally by a
    run 64..70 of the next row (for r = 63 that is the tile corner); the 2 at x = 40 or at
    x = 70.  A weak copy a few rows away is dropped."""
    c = _ones(*F_SHAPE)
    for y0 in (r, 64 + r):
        if y0 + 1 >= F_SHAPE[0]:
            continue
        c[y0, 40:64] = 0
        c[y0 + 1, 64:71] = 0
        if tail2:
            c[y0 + 1, 70] = 2
        else:
            c[y0, 40] = 2
    y1 = r + 4 if r < 32 else r - 4
    c[y1, 40:64] = 0
    c[y1 + 1, 64:71] = 0
    return c


def _comb(down):
    c = _ones(130, 130)
    if down:  # joined by tile row 0 of the second tile row, the teeth into the tile below
        c[64] = 0
        c[65:130, ::2] = 0
        c[129, 20] = 2
        c[0:40, 1::4] = 0  # loose weak teeth above: dropped
    else:  # teeth over rows 0..62, joined by tile row 63
        c[63] = 0
        c[0:63, ::2] = 0
        c[0, 20] = 2
        c[66:100, 1::4] = 0
    return c


def _near_block():
    c = _ones(130, 130)
    c[63, 63] = 2
    c[65:68, 65:68] = 0  # Chebyshev distance 2 of the dot, in the diagonal tile
    c[20, 20] = 2
    c[20:23, 22:25] = 0
    c[100, 64] = 2
    c[101, 63] = 0  # distance 1 over the tile edge: kept
    return c


def _near_ring():
    c = _ones(130, 130)
    for k in (64, 30):
        c[k - 2:k + 3, k - 2:k + 3] = 0
        c[k - 1:k + 2, k - 1:k + 2] = 1
        c[k, k] = 2
    c[100:103, 100:103] = 2  # (something kept)
    c[101, 101] = 1
    return c


def _catalogue():
    cat = []  # (row, name, builder)
    for h, w in A_SHAPES:
        for kind in ("none", "weak", "last2", "strong"):
            cat.append(("a", f"a-{kind}-{h}x{w}", functools.partial(_trivial, kind, h, w)))
    for h, w in I_SHAPES:
        for p in I_P:
            for share in I_SHARE:
                for seed in I_SEEDS:
                    cat.append(("i", f"i-{h}x{w}-p{p}-s{share}-{seed}", functools.partial(_random, h, w, p, share, seed)))
    cat.append(("b", "b-checker-one2", functools.partial(_checker, True)))
    cat.append(("b", "b-checker-no2", functools.partial(_checker, False)))
    cat.append(("c", "c-stripes", _stripes))
    cat.append(("d", "d-serpentine-h", _serpentine))
    cat.append(("d", "d-serpentine-v", lambda: np.ascontiguousarray(_serpentine().T)))
    cat.append(("d", "d-spiral", _spiral))
    for anti in (False, True):
        for end in (0, -1):
            cat.append(("e", f"e-{'anti' if anti else 'main'}diag-end{end}", functools.partial(_diagonal, anti, end)))
    for n, k in ((192, 64), (130, 128)):
        for anti in (False, True):
            for second in (0, 1):
                cat.append(("e", f"e-corner{k}-{'anti' if anti else 'main'}-{second}",
                            functools.partial(_corner_pair, n, k, anti, second)))
    cat.append(("e", "e-south-pairs", _south_diag))
    for y0 in (10, 60):
        cat.append(("f", f"f-px63-y{y0}", functools.partial(_px63, y0)))
    for at in (66, 60):
        cat.append(("f", f"f-run6066-at{at}", functools.partial(_run6066, at)))
    for h in (1, 3):
        for at in (999, 0):
            cat.append(("f", f"f-fullrow-{h}x1000-at{at}", functools.partial(_fullrow, h, at)))
    for r in (0, 1, 62, 63):
        for tail2 in (False, True):
            cat.append(("f", f"f-end63-r{r}-{'tail' if tail2 else 'head'}", functools.partial(_end63, r, tail2)))
    cat.append(("g", "g-comb-up", functools.partial(_comb, False)))
    cat.append(("g", "g-comb-down", functools.partial(_comb, True)))
    cat.append(("h", "h-near-block", _near_block))
    cat.append(("h", "h-near-ring", _near_ring))
    return cat


_CAT = _catalogue()
_BUILD = {name: b for _, name, b in _CAT}
ROW = {name: row for row, name, _ in _CAT}
NAMES = tuple(name for _, name, _ in _CAT)  # benign first: a, i, then the rest
assert len(set(NAMES)) == len(NAMES)


@functools.lru_cache(maxsize=None)
def case(name):
    c = np.ascontiguousarray(_BUILD[name](), np.uint8)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    e, m = reference(case(name))
    e.setflags(write=False)
    m.setflags(write=False)
    return e, m


def partner(name):
    """Another case of the same shape (the next one in the catalogue, cyclically); a p = 0.3
    random map of that shape where the case is the only one of its shape."""
    shape = case(name).shape
    i = NAMES.index(name)
    for other in NAMES[i + 1:] + NAMES[:i]:
        if case(other).shape == shape:
            return case(other)
    return _random(shape[0], shape[1], 0.3, 0.05, 5)


def batch(name):
    """(classes 3 x h x w, edges, mask): an all-1 image, the case, its partner."""
    c, p = case(name), partner(name)
    cls = np.stack([np.ones_like(c), c, p])
    ee, mm = zip(*(reference(x) for x in (cls[0], p)))
    e, m = expected(name)
    return cls, np.stack([ee[0], e, ee[1]]), np.stack([mm[0], m, mm[1]])
