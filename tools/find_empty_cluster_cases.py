#!/usr/bin/env python3
"""Search for key sets on which cv2.kmeans moves a point into an empty cluster.

OpenCV gives a cluster that lost all its points the farthest point of the biggest cluster.
On the colour path's inputs that happens in about one of 10^5 (key set, seed) pairs, so the
cases of tests/empty_cluster_cases.py are found by search: this tool draws small key sets and
runs the CPU oracle (oracle/llfe_oracle.c, exact_sums=1) on each, and prints every set on
which some attempt moves a point, as a literal that can be pasted into the case module.

CPU only and deterministic: worker w of generator g and cluster count K draws from the
splitmix64 stream (base_seed, g, K, w) and makes a fixed number of runs; no time limit, so two
runs with the same arguments print the same cases in the same order.  The draw-and-run loop is
orc_search_empty_cluster (its comment lists the generators: uniform, near-one-dimensional, small
lattice, N in 300 .. 700); up to 16 worker processes run it.

Each hit is re-run through oracle.kmeans_attempts with the float32 and the exact sums and
printed with what it reaches:

    K, N, s (the cv::RNG state is image_rng_state(seed, index) with seed + index = s),
    moves / most moves in one update / moves among equally far points, per attempt,
    iterations per attempt, the winning attempt, and the flags
      f32     the float32 sums give other attempts than the exact ones (not usable: exact
              equality with the device is then not owed)
      near    two attempts' compactnesses are unequal but within 1e-6 relative (not usable)
      two     an attempt with two moves in one update
      tie     a move decided among equally far points
      wins    the moving attempt wins
      big     N > 256

usage: find_empty_cluster_cases.py [--runs R] [--workers W] [--procs P] [--gens 0,1,2,3]
                                   [--ks 4,8,32] [--seed S] [--kinds two,tie,wins,big]
"""
from __future__ import annotations

import argparse
import multiprocessing as mp
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GENS = ("uniform", "line", "lattice", "large")
NEAR_TIE = 1e-6  # tests/colour_cases.py


def _work(job):
    from oracle import oracle

    gen, K, w, runs, base = job
    stream = int(np.random.RandomState([base, gen, K, w]).randint(0, 2 ** 31 - 1, 2, dtype=np.int64) @ [2 ** 31, 1])
    hits, done = oracle.search_empty_cluster(gen, K, stream, runs, max_hits=4096)
    assert done == runs, "hit buffer full: fewer runs per worker"
    return gen, K, w, done, hits


def describe(hit):
    """-> (flags, oracle result) of one hit."""
    from oracle import oracle

    st = oracle.image_rng_state(hit["s"], 0)
    ex = oracle.kmeans_attempts(hit["keys"], hit["K"], st, exact_sums=True)
    f32 = oracle.kmeans_attempts(hit["keys"], hit["K"], st, exact_sums=False)
    assert ex["relocations"].tolist() == hit["relocations"]
    flags = []
    if not all(np.array_equal(ex[f], f32[f]) for f in ("pp", "iters", "att_centers", "att_counts", "att_compactness")):
        flags.append("f32")
    comp = np.sort(ex["att_compactness"])
    gaps = np.diff(comp)
    if np.any((gaps > 0) & (gaps <= NEAR_TIE * comp[:-1])):
        flags.append("near")
    if max(hit["relocations_max"]) >= 2:
        flags.append("two")
    if max(hit["relocation_ties"]) > 0:
        flags.append("tie")
    if hit["relocations"][hit["winner"]] > 0:
        flags.append("wins")
    if len(hit["keys"]) > 256:
        flags.append("big")
    return flags, ex


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=2_000_000, help="runs per worker")
    ap.add_argument("--workers", type=int, default=2, help="workers per (generator, K)")
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--gens", default="0,1,2,3")
    ap.add_argument("--ks", default="2,3,4,5,6,8,32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--kinds", default="", help="print only hits with one of these flags")
    a = ap.parse_args()
    gens = [int(g) for g in a.gens.split(",")]
    ks = [int(k) for k in a.ks.split(",")]
    kinds = set(a.kinds.split(",")) - {""}
    jobs = [(g, K, w, a.runs, a.seed) for g in gens for K in ks for w in range(a.workers)]
    with mp.Pool(min(a.procs, 16, len(jobs))) as pool:
        results = pool.map(_work, jobs, chunksize=1)  # (in job order, whatever finishes first)
    total = 0
    for gen, K, w, done, hits in results:
        total += done
        print(f"# {GENS[gen]} K={K} worker {w}: {done} pairs, {len(hits)} hits")
        for h in hits:
            flags, ex = describe(h)
            if kinds and not kinds & set(flags):
                continue
            moving = [i for i, r in enumerate(h["relocations"]) if r]
            print(f"# {GENS[gen]} N={len(h['keys'])} moving attempts {moving} winner {h['winner']} "
                  f"flags {','.join(flags) or '-'}")
            print(f"#   relocations {h['relocations']} max {h['relocations_max']} ties {h['relocation_ties']}")
            print(f"#   iters {h['iters']}")
            print(f"({h['K']}, {h['s']}, 0, \"{' '.join('%06x' % k for k in h['keys'])}\"),")
    print(f"# {total} pairs searched")


if __name__ == "__main__":
    main()
