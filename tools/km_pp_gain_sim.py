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

The split of owned straddling cubes (DESIGN.md §3 "k-means++: owned straddling cubes split in
place"; kmeans.hip split_owned / gain_signs) is modelled batch by batch as the sweeps form their
64-cube batches (`split_round`): the cube table in the device's order, the cells path's list of the
failing cells' cubes per 64-cell batch and partition, the cubes-only sweep's 64 consecutive cubes per
partition; a cells-path batch with at least SPLIT_MIN owned failing cubes sums those in place, everything
else that fails is summed one by one (the cubes-only sweep of a table below CELL_MIN cubes does not
split, SPLIT_CUBES_ONLY: measured slower on the ui class; the model still reports its batch density).  Printed after the rules above: colours one by one before
and after the split, the owned share of the undecided cubes' colours, undecided trials per owned
cube and the batch density.  `attempt_rounds` restates generateCentersPP's draws (cv::RNG) on a
key list, so tests can ask the model about the exact image and seed they run on the device.

    python tools/km_pp_gain_sim.py [images] [attempts] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = {"cube": (2, 2, 2), "cell": (2, 3, 3), "sup": (2, 4, 4)}  # log2 of the box extents (R, G, B)
COST_BOX, COST_PT = 100.0 / 64.0, 44.0 / 64.0                      # wave-instructions per box test / colour
CELL_MIN = 8192   # kmeans.hip LLFE_KM_CELL_MIN: cube count from which the sweeps take cells first
SPLIT_MIN = 8     # kmeans.hip LLFE_KM_PP_SPLIT_MIN: owned failing cubes of a batch from which they are split
SPLIT_CUBES_ONLY = False  # the cubes-only sweep (tables below CELL_MIN cubes) keeps the one-by-one path


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


def classify(o, e, ch, tr):
    """Per box (origins o, extents - 1 e): owned, A[j], B[j] (box_vals of kmeans.hip)."""
    Dc = (ch * ch).sum(1)[None, :] - 2 * o @ ch.T
    k = (Dc - (ch @ e)[None, :]).argmin(1)
    ck, Dk = ch[k], Dc[np.arange(len(o)), k]
    MK = 2 * (np.maximum(ch[None, :, :] - ck[:, None, :], 0) * e).sum(-1)
    ok = Dc - Dk[:, None] - MK >= 0
    ok[np.arange(len(o)), k] = True
    owned = ok.all(1)
    A, B = np.zeros((len(o), len(tr)), bool), np.zeros((len(o), len(tr)), bool)
    for j, t in enumerate(tr):
        f = (t * t).sum() - 2 * o @ t - Dk
        A[:, j] = f - 2 * (np.maximum(t[None, :] - ck, 0) * e).sum(1) >= 0
        B[:, j] = f + 2 * (np.maximum(ck - t[None, :], 0) * e).sum(1) <= 0
    return owned, A, B


class CubeTable:
    """The device's cube and cell tables of the colours p (n x 3 ints): cubes partition by partition
    (red quarter R), within a partition in (G2, B2, j, c) order (llfe_internal.h CellEnt), cells in
    (R, G2, B2) order with their first cube and cube count."""

    def __init__(self, p):
        R, G, B = p[:, 0] >> 2, p[:, 1] >> 2, p[:, 2] >> 2
        okey = (R << 12) | ((G >> 1) << 7) | ((B >> 1) << 2) | ((G & 1) << 1) | (B & 1)
        self.okey, self.n = np.unique(okey, return_counts=True)
        k = self.okey
        self.o = np.stack([k >> 12, (((k >> 7) & 31) << 1) | ((k >> 1) & 1), (((k >> 2) & 31) << 1) | (k & 1)], 1) * 4
        self.part = k >> 12
        self.cell_id, self.cell_first, self.cell_cubes = np.unique(k >> 2, return_index=True, return_counts=True)
        c = self.cell_id
        self.cell_o = np.stack([(c >> 10) * 4, ((c >> 5) & 31) * 8, (c & 31) * 8], 1)
        self.cell_part = c >> 10


def split_round(tab, ch, tr, split_min=SPLIT_MIN, cells=None, split_cubes_only=SPLIT_CUBES_ONLY):
    """One round's sweep over the table `tab` with chosen centres ch and trials tr -> dict of
    pts_before (colours one by one without the split), pts (with it), split_cubes, split_pts,
    owned_pts (colours of owned undecided cubes), und (undecided trials per owned undecided cube),
    dens (owned undecided cubes per batch that has any), batches_split, und_split (undecided trials
    per split cube), split_idx (the split cubes' indices in the table)."""
    ch, tr = np.asarray(ch, np.int64), np.asarray(tr, np.int64)
    if cells is None:
        cells = len(tab.n) >= CELL_MIN
    owned, A, B = classify(tab.o, np.array([3, 3, 3]), ch, tr)
    fail = ~(A | (owned[:, None] & B)).all(1)
    so = fail & owned
    und = (~A & ~B).sum(1)
    batches = []  # index arrays into the cube table, one per 64-cube batch
    if cells:
        cown, cA, cB = classify(tab.cell_o, np.array([3, 7, 7]), ch, tr)
        cfail = ~(cA | (cown[:, None] & cB)).all(1)
        for b0 in range(0, len(tab.cell_id), 64):
            sl = slice(b0, b0 + 64)
            for P in np.unique(tab.cell_part[sl]):
                m = np.nonzero(cfail[sl] & (tab.cell_part[sl] == P))[0] + b0
                if len(m) == 0:
                    continue
                q = np.concatenate([np.arange(tab.cell_first[i], tab.cell_first[i] + tab.cell_cubes[i]) for i in m])
                batches += [q[i:i + 64] for i in range(0, len(q), 64)]
    else:
        for b0 in range(0, len(tab.n), 64):
            q = np.arange(b0, min(b0 + 64, len(tab.n)))
            batches += [q[tab.part[q] == P] for P in np.unique(tab.part[q])]
    r = {"pts_before": 0, "pts": 0, "split_cubes": 0, "split_pts": 0, "owned_pts": 0, "und": np.zeros(4, np.int64),
         "dens": [], "batches_split": 0, "und_split": np.zeros(4, np.int64), "split_idx": []}
    for q in batches:
        f, s = q[fail[q]], q[so[q]]
        r["pts_before"] += int(tab.n[f].sum())
        r["owned_pts"] += int(tab.n[s].sum())
        r["und"] += np.bincount(und[s], minlength=4)[:4]
        if len(s):
            r["dens"].append(len(s))
        if len(s) >= split_min and (cells or split_cubes_only):
            r["split_cubes"] += len(s)
            r["split_pts"] += int(tab.n[s].sum())
            r["batches_split"] += 1
            r["und_split"] += np.bincount(und[s], minlength=4)[:4]
            r["split_idx"] += s.tolist()
            r["pts"] += int(tab.n[f].sum() - tab.n[s].sum())
        else:
            r["pts"] += int(tab.n[f].sum())
    return r


MASK64 = (1 << 64) - 1


def _cvrng_next(st):
    st[0] = ((st[0] & 0xFFFFFFFF) * 4164903690 + (st[0] >> 32)) & MASK64
    return st[0] & 0xFFFFFFFF


def _cvrng_double(st):
    t = _cvrng_next(st)
    return float((t << 32) | _cvrng_next(st)) * 5.4210108624275221700372640043497e-20


def attempt_rounds(keys, K, rng_state, attempts=10):
    """generateCentersPP (OpenCV kmeans.cpp, 3 trials) on the unique colours `keys` (packed RGB,
    np.unique order) for `attempts` consecutive attempts of the cv::RNG stream `rng_state`:
    -> per attempt (centres K x 3, [(chosen so far, the round's 3 trials) for rounds 1 .. K-1]).
    Distances are exact integers, so the draw p lands on the first i with prefix(D, i) >= p."""
    keys = np.asarray(keys, np.int64)
    p = np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1)
    st = [int(rng_state) or 0xFFFFFFFF]
    out = []
    for _ in range(attempts):
        ch = p[_cvrng_next(st) % len(p)][None, :]
        D = ((p - ch[0]) ** 2).sum(1)
        rounds = []
        for _k in range(1, K):
            s0 = float(D.sum())
            cs = np.cumsum(D)
            tr = []
            for _j in range(3):
                i = int(np.searchsorted(cs, _cvrng_double(st) * s0, side="left"))
                tr.append(p[min(i, len(p) - 1)])
            tr = np.array(tr)
            rounds.append((ch.copy(), tr))
            T = [np.minimum(D, ((p - t) ** 2).sum(1)) for t in tr]
            b = int(np.argmin([int(x.sum()) for x in T]))  # (first minimum)
            D, ch = T[b], np.vstack([ch, tr[b]])
        out.append((ch, rounds))
    return out


def attempts_split(keys, K, rng_state, attempts=10, split_min=SPLIT_MIN):
    """The split model summed over the rounds 1 .. K-1 of every attempt (round 1 is in closed form on
    the device and sweeps nothing: the rounds with chosen centres are those with 1 .. K-1 centres)."""
    keys = np.asarray(keys, np.int64)
    tab = CubeTable(np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1))
    res = []
    for ch, rounds in attempt_rounds(keys, K, rng_state, attempts):
        tot = None
        for c, tr in rounds:
            r = split_round(tab, c, tr, split_min)
            if tot is None:
                tot = r
            else:
                for k in r:
                    tot[k] = tot[k] + r[k]
        res.append((ch, tot))
    return res


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
            tab = CubeTable(p)
            spl = {"pts_before": 0, "pts": 0, "split_cubes": 0, "split_pts": 0, "owned_pts": 0, "und": np.zeros(4, np.int64),
                   "dens": [], "batches_split": 0, "und_split": np.zeros(4, np.int64), "split_idx": []}
            rng = np.random.default_rng(seed + 1000 * i)
            for a in range(n_att):
                ch = p[rng.integers(len(p))][None, :]
                D = ((p - ch[0]) ** 2).sum(1)
                for kk in range(1, 5):
                    tr = p[rng.choice(len(p), 3, p=D / D.sum())]
                    for v, (lv, rule) in enumerate(plans):
                        tot[kk, v] += walk(lv, rule, ch, tr)
                    r = split_round(tab, ch, tr)
                    for key in spl:
                        spl[key] = spl[key] + r[key]
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
            d = np.array(spl["dens"]) if spl["dens"] else np.zeros(1, np.int64)
            in8 = d[d >= SPLIT_MIN].sum() / max(d.sum(), 1)
            print(f"  split of owned undecided cubes (batches of 64, threshold {SPLIT_MIN}): colours one by one"
                  f" {spl['pts_before'] / n_att / U:.3f} U -> {spl['pts'] / n_att / U:.3f} U;"
                  f" owned share {spl['owned_pts'] / max(spl['pts_before'], 1):.2f};"
                  f" {spl['split_cubes'] / n_att:.0f} cubes / {spl['split_pts'] / n_att / U:.3f} U split per attempt")
            print(f"    undecided trials per owned undecided cube 1/2/3: {spl['und'][1]}/{spl['und'][2]}/{spl['und'][3]};"
                  f" owned undecided cubes per batch that has any: mean {d.mean():.1f}, median {np.median(d):.0f};"
                  f" share of them in batches with >= {SPLIT_MIN}: {in8:.2f}")


if __name__ == "__main__":
    main()
