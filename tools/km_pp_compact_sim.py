#!/usr/bin/env python3
"""CPU model, NOT a GPU number: how many 64-lane walks (gain_signs passes) the k-means++ sweeps of kmeans.hip
need for the owned straddling cubes they split, walked inside their own 64-cube batch (before) and from a
per-wave list 64 at a time (DESIGN.md §3 "k-means++: split cubes walked 64 at a time").

Which cubes are split is the rule of tools/km_pp_gain_sim.py `split_round` unchanged (cells path, a batch
with at least SPLIT_MIN owned failing cubes with an undecided trial); `compact_round` forms the same batches
and additionally keeps, per batch, the 64-cell chunk it came from.  A walk is one pass of the 64 positions by
a wave, one trial per live lane; a cube with two or three undecided trials needs a second and a third.

* per batch (before): a split batch walks its own cubes and repeats the pass while a lane has a further
  trial: as many walks as the largest number of undecided trials, live lanes = the sum of the cubes'
  undecided trials;
* per-wave lists: the split cubes are appended to the list of the wave that swept their chunk, a walk runs
  whenever 64 are pending (first in, first out) and takes one trial of each; a cube with a further trial is
  appended again (kmeans.hip pp_walk), so a walk of a full list has 64 live lanes.  At the end of the
  round's sweep each wave walks what is left, at most three partial walks.  The live lanes are the same
  sum.  `mixed` counts the walks whose cubes lie in more than one red-quarter partition.

The device's waves draw runs of LLFE_KM_PPRUN = 4 chunks from a shared counter, so which wave sweeps which
run depends on timing.  The model deals the runs round-robin (run r to wave r mod W): its walk counts are
estimates of the device's, its cubes and live lanes are exact.

    python tools/km_pp_compact_sim.py [images] [attempts] [seed]

`images` bench photos (indices 1, 3, ...) at 1080p with the bench's noise model.  `attempts_compact` is what
the tests use on small images.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.km_pp_gain_sim import CELL_MIN, SPLIT_MIN, CubeTable, attempt_rounds, classify, colours  # noqa: E402

PP_RUN = 4      # kmeans.hip LLFE_KM_PPRUN: 64-cell chunks per work grab
WAVES = (4, 8)  # waves per workgroup of the two builds


def compact_round(tab, ch, tr, split_min=SPLIT_MIN, cells=None):
    """One round's sweep -> dict: split_cubes, split_pts, split_idx, und_split (as split_round's), dens (owned
    undecided cubes per batch that has any), batches_split, lanes (sum of the split cubes' undecided trials),
    old_walks (walks per batch), and per wave count W walks[W], partial[W] (walks below 64 live lanes),
    mixed[W]; round_cubes = [split_cubes] (summed over rounds: the list of the rounds' counts -- a round
    that lists fewer than 64 cubes in all has only partial walks whichever wave sweeps what)."""
    ch, tr = np.asarray(ch, np.int64), np.asarray(tr, np.int64)
    if cells is None:
        cells = len(tab.n) >= CELL_MIN
    r = {"split_cubes": 0, "split_pts": 0, "split_idx": [], "und_split": np.zeros(4, np.int64), "dens": [],
         "batches_split": 0, "lanes": 0, "old_walks": 0, "walks": {w: 0 for w in WAVES},
         "partial": {w: 0 for w in WAVES}, "mixed": {w: 0 for w in WAVES}}
    if not cells:  # the cubes-only sweep does not split: nothing is listed
        r["round_cubes"] = [0]
        return r
    owned, A, B = classify(tab.o, np.array([3, 3, 3]), ch, tr)
    so = ~(A | (owned[:, None] & B)).all(1) & owned
    und = (~A & ~B).sum(1)
    cown, cA, cB = classify(tab.cell_o, np.array([3, 7, 7]), ch, tr)
    cfail = ~(cA | (cown[:, None] & cB)).all(1)
    pend = {w: [[] for _ in range(w)] for w in WAVES}

    def walk(w, pl):  # the first <= 64 entries (cube, trials left) of the list pl
        q = pl[:64]
        del pl[:64]
        r["walks"][w] += 1
        r["partial"][w] += len(q) < 64
        r["mixed"][w] += len(np.unique(tab.part[[i for i, _ in q]])) > 1
        pl += [(i, u - 1) for i, u in q if u > 1]

    for chunk, b0 in enumerate(range(0, len(tab.cell_id), 64)):
        sl = slice(b0, b0 + 64)
        for P in np.unique(tab.cell_part[sl]):
            m = np.nonzero(cfail[sl] & (tab.cell_part[sl] == P))[0] + b0
            if len(m) == 0:
                continue
            q = np.concatenate([np.arange(tab.cell_first[i], tab.cell_first[i] + tab.cell_cubes[i]) for i in m])
            for i in range(0, len(q), 64):
                s = q[i:i + 64]
                s = s[so[s]]
                if len(s):
                    r["dens"].append(len(s))
                if len(s) < split_min:
                    continue
                r["split_cubes"] += len(s)
                r["split_pts"] += int(tab.n[s].sum())
                r["split_idx"] += s.tolist()
                r["und_split"] += np.bincount(und[s], minlength=4)[:4]
                r["batches_split"] += 1
                r["lanes"] += int(und[s].sum())
                r["old_walks"] += int(und[s].max())
                for w in WAVES:
                    pl = pend[w][(chunk // PP_RUN) % w]
                    pl += [(int(i), int(und[i])) for i in s]
                    while len(pl) >= 64:
                        walk(w, pl)
    for w in WAVES:
        for pl in pend[w]:
            while pl:
                walk(w, pl)
    r["round_cubes"] = [r["split_cubes"]]
    return r


def _add(tot, r):
    if tot is None:
        return r
    for k in r:
        tot[k] = {w: tot[k][w] + r[k][w] for w in r[k]} if isinstance(r[k], dict) else tot[k] + r[k]
    return tot


def attempts_compact(keys, K, rng_state, attempts=10, split_min=SPLIT_MIN):
    """compact_round summed over the rounds 1 .. K-1 of every attempt: -> per attempt (centres, dict)."""
    keys = np.asarray(keys, np.int64)
    tab = CubeTable(np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], 1))
    res = []
    for ch, rounds in attempt_rounds(keys, K, rng_state, attempts):
        tot = None
        for c, tr in rounds:
            tot = _add(tot, compact_round(tab, c, tr, split_min))
        res.append((ch, tot))
    return res


def main():
    n_img = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    n_att = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 2025
    print("NumPy model of the k-means++ sweeps' split batches: not a GPU number.  Runs of 4 chunks dealt round-robin.")
    for i in [2 * j + 1 for j in range(n_img)]:
        p = colours(i, seed, "photo")
        keys = (p[:, 0] << 16) | (p[:, 1] << 8) | p[:, 2]
        tab = CubeTable(p)
        print(f"photo image {i}: U={len(p)} cubes={len(tab.n)} cells={len(tab.cell_id)}"
              f" ({'cells path' if len(tab.n) >= CELL_MIN else 'cubes only: no lists'})")
        tot = None
        for a, (_, t) in enumerate(attempts_compact(keys, 5, 0x9E3779B97F4A7C15 ^ (seed + i), n_att)):
            d = np.array(t["dens"]) if t["dens"] else np.zeros(1, np.int64)
            print(f"  attempt {a}: {t['split_cubes']} cubes split in {t['batches_split']} batches, undecided trials 1/2/3"
                  f" {t['und_split'][1]}/{t['und_split'][2]}/{t['und_split'][3]}, live lanes {t['lanes']};"
                  f" owned undecided cubes per batch that has any: mean {d.mean():.1f}")
            print(f"    per batch: {t['old_walks']} walks at {t['lanes'] / max(t['old_walks'], 1):.1f} live lanes")
            for w in WAVES:
                print(f"    per-wave lists, {w} waves: {t['walks'][w]} walks at {t['lanes'] / max(t['walks'][w], 1):.1f} live lanes"
                      f" ({t['partial'][w]} partial, {t['mixed'][w]} over more than one partition)")
            tot = _add(tot, {k: v for k, v in t.items() if k not in ("dens", "split_idx", "round_cubes")})
        print(f"  per attempt: {tot['split_cubes'] / n_att:.0f} cubes; per batch {tot['old_walks'] / n_att:.0f} walks at"
              f" {tot['lanes'] / max(tot['old_walks'], 1):.1f} live lanes; " +
              "; ".join(f"{w} waves {tot['walks'][w] / n_att:.0f} walks at {tot['lanes'] / max(tot['walks'][w], 1):.1f}"
                        f" ({tot['old_walks'] / max(tot['walks'][w], 1):.2f} x fewer)" for w in WAVES))


if __name__ == "__main__":
    main()
