#!/usr/bin/env python3
"""CPU simulation: what the k-means++ sweeps of kmeans.hip (pp_cubes) test and sum one by one
per round, under the rule that sums T_j = sum min(D, d(., t_j)) and under the gain form
g_j = sum max(0, D - d(., t_j)), T_j = sum(D) - g_j (DESIGN.md §3 "k-means++ on cubes").

A NumPy model of the kernel's decision rules with its corner margins, on the bench's synthetic
images (1080p, noise trunc(N(0, 0.5)) per channel), D^2-proportional trial draws, rounds 1-4:

* box levels: 4 x 4 x 4 cubes, 4 x 8 x 8 cells, 4 x 16 x 16 super-cells (R x G x B), non-empty
  boxes only; owner candidate k = the chosen centre nearest to the box centre; `owned` = no
  other chosen centre is ever strictly closer on the box; A_j = trial j never strictly closer
  than c_k, B_j = always at least as close (linear forms at the origin -/+ the corner margin);
* sums rule ("current"): a box is decided when owned and every trial is A or B;
* gain form: a box is decided when every trial is A (gain 0, owned or not) or owned and B;
* an undecided super-cell hands its cells to the cell level, an undecided cell its cubes to
  the cube level, an undecided cube's colours are summed one by one.

Printed per round: box tests and colours one by one for (a) the sums rule with cells -> cubes
(what rounds >= 1 ran before), (b) the gain form with cells -> cubes, (c) the gain form with
super-cells -> cells -> cubes; then a wave-instruction estimate at 100 per 64 box tests and 44
per 64 colours.  Not a GPU measurement.

    python tools/km_pp_gain_sim.py [images] [attempts] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = {"cube": (2, 2, 2), "cell": (2, 3, 3), "sup": (2, 4, 4)}  # log2 of the box extents (R, G, B)
COST_BOX, COST_PT = 100.0 / 64.0, 44.0 / 64.0                      # wave-instructions per box test / colour


def colours(i, seed, kind):
    from low_level_feature_extraction_amd import synth

    bgr = synth.synth_numpy(i, 1080, 1920, seed=seed, kind=kind)
    rng = np.random.default_rng(seed + i)
    rgb = bgr[..., ::-1].reshape(-1, 3).astype(np.int16)
    rgb = np.clip(rgb + np.trunc(rng.normal(0, 0.5, rgb.shape)).astype(np.int16), 0, 255).astype(np.int64)
    keys = np.unique((rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2])
    return np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1)


class Boxes:
    """The non-empty boxes of one level: origins, extents - 1, colour counts, parent index."""

    def __init__(self, p, shifts, parent_shifts=None):
        sh = np.array(shifts)
        b = p >> sh
        bid = (b[:, 0] << 16) | (b[:, 1] << 8) | b[:, 2]
        self.ids, self.inv, self.n = np.unique(bid, return_inverse=True, return_counts=True)
        self.o = np.stack([(self.ids >> 16) & 255, (self.ids >> 8) & 255, self.ids & 255], 1) << sh
        self.ext = (1 << sh) - 1
        self.parent = None
        if parent_shifts is not None:
            pb = self.o >> np.array(parent_shifts)
            pid = (pb[:, 0] << 16) | (pb[:, 1] << 8) | pb[:, 2]
            self.parent = np.unique(pid, return_inverse=True)[1]  # (parents: the same ascending ids)


def decide(bx, ch, tr):
    """-> (decided under the sums rule, decided under the gain form) per box."""
    o, e = bx.o, bx.ext
    Dc = (ch * ch).sum(1)[None, :] - 2 * o @ ch.T            # D_m(o) = |c_m|^2 - 2 o.c_m
    k = (Dc - (ch @ e)[None, :]).argmin(1)                   # nearest to the box centre (first minimum)
    ck, Dk = ch[k], Dc[np.arange(len(o)), k]
    MK = 2 * (np.maximum(ch[None, :, :] - ck[:, None, :], 0) * e).sum(-1)
    ok = Dc - Dk[:, None] - MK >= 0
    ok[np.arange(len(o)), k] = True
    owned = ok.all(1)
    cur = owned.copy()
    gain = np.ones(len(o), bool)
    for t in tr:
        f = (t * t).sum() - 2 * o @ t - Dk
        A = f - 2 * (np.maximum(t[None, :] - ck, 0) * e).sum(1) >= 0
        B = f + 2 * (np.maximum(ck - t[None, :], 0) * e).sum(1) <= 0
        cur &= A | B
        gain &= A | (owned & B)
    return cur, gain


def walk(levels, rule, ch, tr):
    """Box tests and colours summed one by one walking `levels` (coarse -> cube)."""
    tests, live = 0, None
    for j, bx in enumerate(levels):
        dec = decide(bx, ch, tr)[rule]
        cand = np.ones(len(bx.o), bool) if live is None else live[bx.parent]
        tests += int(cand.sum())
        live = cand & ~dec
        if j + 1 < len(levels):
            assert levels[j + 1].parent.max() == len(bx.o) - 1
    return tests, int(levels[-1].n[live].sum())


def main():
    n_img = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    n_att = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 2025
    names = ("sums, cells->cubes", "gain, cells->cubes", "gain, sups->cells->cubes")
    for kind, idx in [("photo", [2 * i + 1 for i in range(n_img)]), ("ui", [0])]:
        for i in idx:
            p = colours(i, seed, kind)
            cube = Boxes(p, LEVELS["cube"], LEVELS["cell"])
            cell = Boxes(p, LEVELS["cell"], LEVELS["sup"])
            sup = Boxes(p, LEVELS["sup"])
            # (the device takes cells / super-cells from 8 192 cubes on; smaller tables walk cubes only)
            hier = len(cube.o) >= 8192
            plans = [([cell, cube] if hier else [cube], 0), ([cell, cube] if hier else [cube], 1),
                     ([sup, cell, cube] if hier else [cube], 1)]
            tot = np.zeros((5, 3, 2), np.int64)
            rng = np.random.default_rng(seed + 1000 * i)
            for a in range(n_att):
                ch = p[rng.integers(len(p))][None, :]
                D = ((p - ch[0]) ** 2).sum(1)
                for kk in range(1, 5):
                    tr = p[rng.choice(len(p), 3, p=D / D.sum())]
                    for v, (lv, rule) in enumerate(plans):
                        tot[kk, v] += walk(lv, rule, ch, tr)
                    T = [np.minimum(D, ((p - t) ** 2).sum(1)) for t in tr]
                    b = int(np.argmin([x.sum() for x in T]))
                    D, ch = T[b], np.vstack([ch, tr[b]])
            U = len(p)
            print(f"{kind} image {i}: U={U} cubes={len(cube.o)} cells={len(cell.o)} super-cells={len(sup.o)}"
                  f" ({n_att} attempts, per attempt)")
            for kk in range(1, 5):
                print(f"  round {kk}: " + "; ".join(f"{names[v]}: {tot[kk, v, 0] / n_att:.0f} tests / {tot[kk, v, 1] / n_att:.0f} colours"
                                                     for v in range(3)))
            s = tot[1:].sum(0) / n_att
            base = s[0, 0] * COST_BOX + s[0, 1] * COST_PT
            for v in range(3):
                est = s[v, 0] * COST_BOX + s[v, 1] * COST_PT
                print(f"  rounds 1-4, {names[v]}: {s[v, 0]:.0f} tests / {s[v, 1]:.0f} colours ({s[v, 1] / U:.3f} U);"
                      f" wave-instruction estimate {est:.0f} ({est / base:.2f} of the sums rule)")


if __name__ == "__main__":
    main()
