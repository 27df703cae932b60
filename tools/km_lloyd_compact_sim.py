#!/usr/bin/env python3
"""CPU model, NOT a GPU number: how the Lloyd cube sweep of kmeans.hip (cells path) forms its 64-cube
batches and how many 64-lane bisector walks its two-centre cubes need (DESIGN.md §3 "Two-centre cubes
walked 64 at a time").

A NumPy restatement of the sweep's batch formation on one image's unique colours: super-cells
(4 x 16 x 16, 64 per chunk, in table order) -> the failing super-cells' cells (4 x 8 x 8, 64 per batch)
-> the failing cells' cubes (4 x 4 x 4, 64 per batch), each level with the device's margin test (owner
k = first minimum at the box centre, pass when d_j - d_k > 3 |dx| + e (|dy| + |dz|) + 1 for every other
centre j, e = 3 / 7 / 15) but in float64, from float64 Lloyd centres (means of the float64 labelling,
k-means++ centres from `attempt_rounds`, OpenCV's stop rule).  The device's margins and centres are
float32 and an edge case may fall on either side, so the counts are estimates of the device's, not its
counters.  A failing cube with exactly one contender is a two-centre cube, one with more goes to the
colour ring whole.

Per Lloyd iteration it reports the cube batches, the two-centre and multi-contender cubes, then

* the per-batch rule (before): a batch with at least 12 two-centre cubes walks them in its own batch --
  walks and live lanes per walk, and the two-centre cubes of the batches below the threshold;
* per-wave lists: every two-centre cube is appended to the list of the wave that drew its super-cell chunk
  (chunks dealt round-robin here; the device's waves draw them from a counter), a walk runs whenever 64 are
  pending and one partial walk per wave flushes the rest at the sweep's end -- walks, the partial ones
  among them and live lanes per walk, for 4 and for 8 waves.

    python tools/km_lloyd_compact_sim.py [images] [attempts] [seed]

`images` bench photos (indices 1, 3, ...) at 1080p with the bench's noise model, `attempts` k-means
attempts each.  `sweep_counts` / `attempt_counts` are what the tests use on small images.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.km_pp_gain_sim import CubeTable, attempt_rounds, colours  # noqa: E402

CELL_MIN = 8192    # kmeans.hip LLFE_KM_CELL_MIN: cube count from which the sweep takes super-cells and cells first
OLD_SPLIT_MIN = 12  # the per-batch rule's threshold (LLFE_KM_SPLIT_MIN before the lists)
WAVES = (4, 8)     # waves per workgroup of the two builds


class LloydTables:
    """Cube and cell tables in the device's order (CubeTable) and the super-cells over them: per
    super-cell (ascending R, G4, B4) its cells' indices in cell-table order (the j = 0 pair, then j = 1)."""

    def __init__(self, p):
        self.tab = CubeTable(p)
        c = self.tab.cell_id  # R << 10 | G2 << 5 | B2
        sid = ((c >> 10) << 8) | (((c >> 6) & 15) << 4) | ((c >> 1) & 15)
        order = np.argsort(sid, kind="stable")  # (cell-table order within a super-cell)
        self.sup_id, first, cnt = np.unique(sid[order], return_index=True, return_counts=True)
        self.sup_cells = [order[f:f + n] for f, n in zip(first, cnt)]
        s = self.sup_id
        self.sup_o = np.stack([(s >> 8) * 4, ((s >> 4) & 15) * 16, (s & 15) * 16], 1)


def _box_test(o, half, e, c):
    """Margin test of the boxes with origins o: -> (owner k, contenders: n x K bool, pass)."""
    q = o + np.asarray(half)
    d = ((q[:, None, :] - c[None]) ** 2).sum(-1)
    k = d.argmin(1)
    ck = c[k]
    a = np.abs(c[None, :, :] - ck[:, None, :])
    thr = 3.0 * a[..., 0] + e * (a[..., 1] + a[..., 2]) + 1.0
    cont = d - d[np.arange(len(o)), k][:, None] <= thr
    cont[np.arange(len(o)), k] = False
    return k, cont, ~cont.any(1)


def sweep_counts(lt, c):
    """One Lloyd sweep with centres c (K x 3 float64) over the tables lt -> dict: batches (cube batches),
    two / multi (cubes), old_walks / old_live / old_below (per-batch rule), and per wave count W
    walks[W], partial[W], live[W] (cubes in those walks = every two-centre cube)."""
    tab = lt.tab
    _, _, spass = _box_test(lt.sup_o, (1.5, 7.5, 7.5), 15.0, c)
    _, _, cpass = _box_test(tab.cell_o, (1.5, 3.5, 3.5), 7.0, c)
    _, ccont, qpass = _box_test(tab.o, (1.5, 1.5, 1.5), 3.0, c)
    two = ~qpass & (ccont.sum(1) == 1)
    multi = ~qpass & (ccont.sum(1) > 1)
    r = {"batches": 0, "two": 0, "multi": 0, "old_walks": 0, "old_live": 0, "old_below": 0,
         "walks": {w: 0 for w in WAVES}, "partial": {w: 0 for w in WAVES}, "full_on_nonempty": 0}
    pend = {w: np.zeros(w, np.int64) for w in WAVES}
    for chunk, s0 in enumerate(range(0, len(lt.sup_id), 64)):
        fs = [s for s in range(s0, min(s0 + 64, len(lt.sup_id))) if not spass[s]]
        if not fs:
            continue
        cells = np.concatenate([lt.sup_cells[s] for s in fs])
        for b0 in range(0, len(cells), 64):
            fc = [i for i in cells[b0:b0 + 64] if not cpass[i]]
            if not fc:
                continue
            cubes = np.concatenate([np.arange(tab.cell_first[i], tab.cell_first[i] + tab.cell_cubes[i]) for i in fc])
            for q0 in range(0, len(cubes), 64):
                q = cubes[q0:q0 + 64]
                n2, nm = int(two[q].sum()), int(multi[q].sum())
                r["batches"] += 1
                r["two"] += n2
                r["multi"] += nm
                if n2 >= OLD_SPLIT_MIN:
                    r["old_walks"] += 1
                    r["old_live"] += n2
                else:
                    r["old_below"] += n2
                for w in WAVES:
                    i = chunk % w
                    if w == WAVES[0] and n2 == 64 and pend[w][i] > 0:
                        r["full_on_nonempty"] += 1  # (the list then holds 64 + what was pending)
                    pend[w][i] += n2
                    while pend[w][i] >= 64:
                        pend[w][i] -= 64
                        r["walks"][w] += 1
    for w in WAVES:
        part = int((pend[w] > 0).sum())
        r["walks"][w] += part
        r["partial"][w] = part
    return r


def lloyd_sweeps(p, c0, max_iter=100, eps=0.2):
    """Float64 Lloyd from centres c0 on the colours p: -> the centres of every sweep (OpenCV's stop rule:
    the largest centre move <= eps, or max_iter)."""
    c = np.asarray(c0, np.float64).copy()
    pf = p.astype(np.float64)
    out = []
    for it in range(max_iter):
        out.append(c.copy())
        lab = ((pf[:, None, :] - c[None]) ** 2).sum(-1).argmin(1)
        n = np.bincount(lab, minlength=len(c)).astype(np.float64)
        s = np.stack([np.bincount(lab, pf[:, d], minlength=len(c)) for d in range(3)], 1)
        new = np.where(n[:, None] > 0, s / np.maximum(n, 1)[:, None], c)  # (an empty cluster keeps its centre here)
        shift = ((new - c) ** 2).sum(1).max()
        c = new
        if it + 1 == max_iter - 1 or shift <= eps * eps:
            break
    return out


def attempt_counts(keys, K, rng_state, attempts=10):
    """Per attempt the list of sweep_counts dicts of its Lloyd sweeps (k-means++ as generateCentersPP)."""
    keys = np.asarray(keys, np.int64)
    p = np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1)
    lt = LloydTables(p)
    return [[sweep_counts(lt, c) for c in lloyd_sweeps(p, ch)] for ch, _ in attempt_rounds(keys, K, rng_state, attempts)]


def main():
    n_img = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    n_att = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 2025
    print("NumPy model of the Lloyd sweep's batches (float64): not a GPU number.")
    for i in [2 * j + 1 for j in range(n_img)]:
        p = colours(i, seed, "photo")
        keys = (p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2]
        lt = LloydTables(p)
        print(f"photo image {i}: U={len(p)} cubes={len(lt.tab.n)} cells={len(lt.tab.cell_id)} super-cells={len(lt.sup_id)}"
              f" ({'cells path' if len(lt.tab.n) >= CELL_MIN else 'cubes only: no lists'})")
        for a, (ch, _) in enumerate(attempt_rounds(keys, 5, 0x9E3779B97F4A7C15 ^ (seed + i), n_att)):
            sw = [sweep_counts(lt, c) for c in lloyd_sweeps(p, ch)]
            n = len(sw)
            tot = lambda f: sum(f(s) for s in sw)  # noqa: E731
            ow, ol = tot(lambda s: s["old_walks"]), tot(lambda s: s["old_live"])
            print(f"  attempt {a}: {n} sweeps; per sweep: {tot(lambda s: s['batches']) / n:.1f} cube batches,"
                  f" {tot(lambda s: s['two']) / n:.0f} two-centre cubes, {tot(lambda s: s['multi']) / n:.0f} multi-contender")
            print(f"    per-batch rule (threshold {OLD_SPLIT_MIN}): {ow / n:.1f} walks at {ol / max(ow, 1):.1f} live lanes,"
                  f" {tot(lambda s: s['old_below']) / n:.0f} two-centre cubes in batches below the threshold")
            for w in WAVES:
                wk, pt = tot(lambda s: s["walks"][w]), tot(lambda s: s["partial"][w])
                print(f"    per-wave lists, {w} waves: {wk / n:.1f} walks ({pt / n:.1f} partial) at"
                      f" {tot(lambda s: s['two']) / max(wk, 1):.1f} live lanes")
            for j, s in enumerate(sw):
                print(f"      sweep {j:2d}: batches {s['batches']:3d} two {s['two']:5d} multi {s['multi']:4d} | per batch:"
                      f" walks {s['old_walks']:3d} live {s['old_live'] / max(s['old_walks'], 1):4.1f} |"
                      + " |".join(f" {w} waves: walks {s['walks'][w]:3d} partial {s['partial'][w]}" for w in WAVES))


if __name__ == "__main__":
    main()
