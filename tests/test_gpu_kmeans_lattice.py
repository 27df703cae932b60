"""The pair-table split of two-centre cubes (csrc/kmeans_lattice.h, read by kmeans.hip's split_drain in
the 256-thread build) on inputs made for its corners.  The table sorts the 16 values gy j' + gz b of a
centre pair and reads each slice's two sides as a suffix and a prefix of that order, so what can go
wrong is the order itself: ties, and the pair read from its larger index.  Four families of small
images (caller noise of zeros, so the unique colours are exactly the ones laid out here; every image
has more than 8 192 cubes, the cells path, the only one that splits):

  one_channel  a slab along R over one pattern of (G, B): K = 2 halves it, and once the halves are
               whole R layers their centres agree in G and B to an ulp: gy = gz = 0, 16 equal values
  diagonal     a band around the G = B diagonal, symmetric under G <-> B: K = 2 cuts across it and
               the centres' G and B steps come out equal: gy = gz, the values tie in anti-diagonals
  three_blobs  three adjacent boxes and K = 3: centres 3 and 4 stay unused, only three tables are built
  reversed     a slab along R, dense below R = 176 and half as dense above: K = 2 cuts it near R = 115, and over
               the ten attempts' sweeps the pair's larger index owns most of the two-centre cubes (58 % on the
               oracle's centres), which the table serves by negation

Every case compares all 10 attempts with the oracle's cv2.kmeans restatement in its exact-sum mode, as
tests/test_gpu_kmeans_bisector.py does: k-means++ centres, iterations, float32 centres and counts equal,
compactness within 1e-6 relative; and reads from the LLFE_KM_TRACE line that cubes were split, so the
lookup ran.  test_families_reach_their_corner checks on the oracle's centres that the inputs do what
the list above says."""
import numpy as np
import pytest

pytestmark = [pytest.mark.timeout(120)]

CELL_MIN = 8192  # kmeans.hip LLFE_KM_CELL_MIN
SEED = 2027
COL_SPLIT_CUBES, COL_SPLIT_PTS = 17, 18  # LLFE_KM_TRACE columns (llfe_pipeline.cpp)


def _image(rgb, side):
    """side x side BGR image holding exactly the colours `rgb` (repeated to fill it), shuffled"""
    rgb = np.asarray(rgb, np.int64)
    assert len(rgb) <= side * side and rgb.min() >= 0 and rgb.max() <= 255
    rs = np.random.RandomState(11)
    fill = rgb[rs.randint(0, len(rgb), side * side - len(rgb))]
    px = np.concatenate([rgb, fill])[rs.permutation(side * side)]
    return np.ascontiguousarray(px[:, ::-1].reshape(side, side, 3).astype(np.uint8))


def _grid(*axes):
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(axes))


def _one_channel():
    gb = _grid(np.arange(104, 152), np.arange(104, 152))
    gb = gb[(gb[:, 0] + gb[:, 1]) % 4 == 0]  # four of every 4 x 4 tile
    r = np.arange(250)
    rgb = np.concatenate([np.repeat(r, len(gb))[:, None], np.tile(gb, (len(r), 1))], 1)
    return _image(rgb, 384), 2


def _diagonal():
    gb = _grid(np.arange(256), np.arange(256))
    gb = gb[(np.abs(gb[:, 0] // 4 - gb[:, 1] // 4) <= 4) & (gb[:, 0] % 4 == gb[:, 1] % 4)]  # symmetric under G <-> B
    r = np.arange(96, 160)
    rgb = np.concatenate([np.repeat(r, len(gb))[:, None], np.tile(gb, (len(r), 1))], 1)
    return _image(rgb, 384), 2


def _box(lo, edge, keep, rs):
    p = _grid(*[np.arange(o, o + edge) for o in lo])
    return p[rs.permutation(len(p))[: len(p) // keep]]


def _three_blobs():
    rs = np.random.RandomState(3)
    rgb = np.concatenate([_box((40, 60, 60), 64, 6, rs), _box((104, 60, 60), 64, 6, rs), _box((72, 124, 60), 64, 6, rs)])
    return _image(rgb, 384), 3


def _reversed():
    gb = _grid(np.arange(104, 152), np.arange(104, 152))
    lo_gb, hi_gb = gb[(gb[:, 0] + gb[:, 1]) % 4 == 0], gb[(gb[:, 0] + gb[:, 1]) % 8 == 0]  # four / two of every 4 x 4 tile
    r0, r1 = np.arange(176), np.arange(176, 256)
    rgb = np.concatenate([np.concatenate([np.repeat(r0, len(lo_gb))[:, None], np.tile(lo_gb, (len(r0), 1))], 1),
                          np.concatenate([np.repeat(r1, len(hi_gb))[:, None], np.tile(hi_gb, (len(r1), 1))], 1)])
    return _image(rgb, 384), 2


CASES = {"one_channel": _one_channel, "diagonal": _diagonal, "three_blobs": _three_blobs, "reversed": _reversed}


@pytest.fixture(scope="module")
def runs(orc):
    """name -> (image, K, noise, unique keys, the oracle's attempts); computed once"""
    out = {}
    for name, make in CASES.items():
        host, k = make()
        h, w = host.shape[:2]
        noise = np.zeros((h * w, 3), np.int8)
        keys = orc.color_unique(host, noise)
        out[name] = (host, k, noise, keys, orc.kmeans_attempts(keys, k, orc.image_rng_state(SEED, 0), exact_sums=True))
    return out


def _two_centre(keys, c):
    """The two-centre cubes of one sweep with centres c (float32 rows): owner k (first minimum at the cube centre)
    and the one contender j that fails its margin row, as the kernel's cube test finds them."""
    c = c.astype(np.float64)
    cube = np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63))
    q = np.stack([(cube >> 12) & 63, (cube >> 6) & 63, cube & 63], -1) * 4.0 + 1.5
    dq = ((q[:, None, :] - c[None]) ** 2).sum(-1)
    k = dq.argmin(1)
    thr = 3.0 * np.abs(c[None, :, :] - c[k][:, None, :]).sum(-1) + 1.0
    cont = dq - dq[np.arange(len(cube)), k][:, None] <= thr
    cont[np.arange(len(cube)), k] = False
    two = cont.sum(1) == 1
    return k[two], cont.argmax(1)[two]


def _steps(c, k, j):
    return np.rint((c[k].astype(np.float32) - c[j].astype(np.float32)) * np.float32(2048)).astype(np.int64)


def test_families_reach_their_corner(runs):
    """On the oracle's centres (every sweep of every attempt): the sweeps in which two-centre cubes meet
    gy = gz = 0 (one_channel), gy = gz != 0 (diagonal), and the share of two-centre cubes owned by the
    pair's larger index (reversed)."""
    seen = {}
    for name, (host, K, noise, keys, ex) in runs.items():
        n_cubes = len(np.unique(((keys >> 18) & 63) << 12 | ((keys >> 10) & 63) << 6 | ((keys >> 2) & 63)))
        assert n_cubes >= CELL_MIN, (name, n_cubes)
        zero = diag = own_hi = own_lo = 0
        for a in range(10):
            sweeps = [ex["pp"][a]] + [ex["iter_centers"][a, i] for i in range(int(ex["iters"][a]) - 1)]
            for cen in sweeps:
                cen = np.asarray(cen)[:K]
                if np.isnan(cen).any():
                    continue
                k, j = _two_centre(keys, cen)
                own_hi += int((k > j).sum())
                own_lo += int((k < j).sum())
                for kk, jj in set(zip(k.tolist(), j.tolist())):
                    g = _steps(cen, kk, jj)
                    n = int(((k == kk) & (j == jj)).sum())
                    zero += n if g[1] == 0 and g[2] == 0 else 0
                    diag += n if g[1] == g[2] != 0 else 0
        seen[name] = (zero, diag, own_hi, own_lo)
        print(f"{name}: cubes {n_cubes}, two-centre cubes met with gy = gz = 0: {zero}, with gy = gz != 0: {diag}, "
              f"owned by the larger index {own_hi}, by the smaller {own_lo}")
    assert seen["one_channel"][0] > 0
    assert seen["diagonal"][1] > 0
    assert seen["reversed"][2] > seen["reversed"][3] > 0


BATCH = 104  # 1 040 attempts: more than the GPU holds at once, so the 256-thread build runs (tests/test_gpu_kmeans_bisector.py)


def _filler():
    """a 384 x 384 image of 16 colours: an attempt on it costs nothing"""
    v = (np.arange(384 * 384) % 16).reshape(384, 384)
    return np.ascontiguousarray(np.stack([v * 16, 255 - v * 16, v * 8 + 64], -1).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_attempts_equal_exact_sum_oracle(backend, runs, tmp_path, monkeypatch, name):
    """The case's image leads a batch of 104 (the rest are 16-colour fillers), so its attempts run in the
    256-thread build, the one that reads the pair tables."""
    host, K, noise, keys, ex = runs[name]
    batch = np.stack([host] + [_filler()] * (BATCH - 1))
    trace = tmp_path / "km_trace.txt"
    monkeypatch.setenv("LLFE_KM_TRACE", str(trace))
    r = backend.process(batch, ("colors",), seed=SEED, noise=np.zeros((BATCH,) + noise.shape, np.int8), index_base=0, n_colors=K)[0]
    att = backend.kmeans_attempts(BATCH)[0]
    assert r.n_unique == len(keys)
    t = np.atleast_2d(np.loadtxt(trace, dtype=np.int64))
    assert t.shape[0] == 10 * BATCH and t.shape[1] > COL_SPLIT_PTS, t.shape
    t = t[t[:, 0] == 0]
    assert t.shape[0] == 10 and (t[:, 2] == len(keys)).all(), t[:, :3]
    n_split, n_split_pts = int(t[:, COL_SPLIT_CUBES].sum()), int(t[:, COL_SPLIT_PTS].sum())
    print(f"{name}: U={len(keys)} K={K} split cubes={n_split} colours decided={n_split_pts} iterations={[a['iters'] for a in att]}")
    for a in range(10):
        assert np.array_equal(att[a]["pp_centers"][:K], ex["pp"][a]), (a, att[a]["pp_centers"], ex["pp"][a])
        assert att[a]["iters"] == int(ex["iters"][a]), (a, att[a]["iters"], ex["iters"][a])
        assert np.array_equal(att[a]["centers"][:K], ex["att_centers"][a]), a
        assert np.array_equal(att[a]["counts"][:K], ex["att_counts"][a]), a
        assert abs(att[a]["compactness"] - ex["att_compactness"][a]) <= 1e-6 * ex["att_compactness"][a], a
    assert n_split > 0 and n_split_pts > 0, (name, n_split, n_split_pts)
