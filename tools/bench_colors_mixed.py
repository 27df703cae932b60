#!/usr/bin/env python
"""The analysis of a batch of device-resident images of any sizes: the colours of all images in
one device pass, and the shapes and shadows as well, against the size-grouped route (DESIGN.md §3
"Colours of a mixed-size batch" and "Shapes and shadows of a mixed-size batch"; figures in
profiles/colors_images/ and profiles/shapes_images/).  bench.py is not touched: this tool measures
the opt-in routes beside it.

  grouped   Backend.process_images(feed, features): one pass per size group
  one_pass  ... colors="one_pass": one colour pass, shapes and shadows by size group
  both      ... colors="one_pass", shapes="one_pass": one colour pass, one shapes / shadows pass

A seeded feed of --images synthetic images (bench.py's generator) on the device, one process, a
warm-up of all, then the three routes alternating for --legs legs each, every leg --reps passes
over the feed, for the features ("colors",) and ("colors", "shapes", "shadows"):
  --feed mixed     16 distinct sizes: the (1920, 1080) thumbnails of bench_thumb.py's mixed feed
  --feed distinct  every image its own size, widths and heights drawn around those thumbnails'
  --feed uniform   every image 1920 x 1080, where the grouped route is at its best
After the timed legs one profiled pass of each route gives the launches and the ms of the colour
kernels, of k_stencil and of k_hysteresis_dilate (llfe_kernel_stats) and the busy time of the host
contour pool (llfe_host_contour_stats).  One JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

COLOUR_KERNELS = ("k_uq_scatter", "k_uq_part", "k_uq_gather", "k_kmeans")
SHAPE_KERNELS = ("k_stencil", "k_hysteresis_dilate")
# route -> (colors=, shapes=) of Backend.process_images
ROUTES = {"grouped": ("grouped", "grouped"), "one_pass": ("one_pass", "grouped"), "both": ("one_pass", "one_pass")}


def feed_sizes(kind: str, n: int, seed: int):
    """(h, w) per image."""
    from low_level_feature_extraction_amd.backend import thumbnail_size
    from tools.bench_thumb import feed_sizes as source_sizes

    if kind == "uniform":
        return [(1080, 1920)] * n
    if kind == "mixed":
        out = []
        for h, w in source_sizes("mixed", n, seed):
            t = thumbnail_size(w, h) or (w, h)
            out.append((t[1], t[0]))
        return out
    r = np.random.default_rng(seed)
    sizes = set()
    while len(sizes) < n:  # aspect ratios between 4:3 and 16:9 at the thumbnail box
        h = int(r.integers(810, 1081))
        sizes.add((h, min(1920, int(h * r.uniform(4 / 3, 16 / 9)))))
    return [sorted(sizes)[i] for i in r.permutation(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feed", choices=("mixed", "distinct", "uniform"), default="mixed")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.legs < 3:
        ap.error("--legs: at least three legs each")

    import torch

    from low_level_feature_extraction_amd import synth
    from low_level_feature_extraction_amd.backend import Backend

    be = Backend.get(0)
    sizes = feed_sizes(args.feed, args.images, args.seed)
    feed = [synth.synth_image(i, h, w, seed=args.seed + 4321, device="cuda:0") for i, (h, w) in enumerate(sizes)]
    routes = tuple(ROUTES)

    def run(route, feats):
        colors, shapes = ROUTES[route]
        return be.process_images(feed, feats, seed=7, index_base=0, colors=colors, shapes=shapes)

    def leg(route, feats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            run(route, feats)
        torch.cuda.synchronize()
        return args.reps * len(feed) / (time.perf_counter() - t0)

    def profiled(route, feats):
        """-> (colour kernels, shape kernels, host contour pool) of one pass over the feed"""
        be.set_profiling(True)
        try:
            before = be.kernel_stats()
            be.host_contour_stats(reset=True)
            t0 = time.perf_counter()
            run(route, feats)
            wall = 1e3 * (time.perf_counter() - t0)
            host = be.host_contour_stats(reset=True)
            st = be.kernel_stats()
        finally:
            be.set_profiling(False)
        zero = {"launches": 0, "total_ms": 0.0}

        def added(names):
            return {k: {"launches": st[k]["launches"] - before.get(k, zero)["launches"],
                        "ms": round(st[k]["total_ms"] - before.get(k, zero)["total_ms"], 3)} for k in names if k in st}

        pool = {"busy_ms": round(host["busy_ms"], 3), "images": host["images"], "threads": host["threads"],
                "call_wall_ms": round(wall, 3)}
        return added(COLOUR_KERNELS), added(SHAPE_KERNELS), pool

    out = {"tool": "bench_colors_mixed", "feed": args.feed, "images": len(feed), "distinct_sizes": len(set(sizes)),
           "reps_per_leg": args.reps, "device": torch.cuda.get_device_name(0), "features": {}}
    for feats in (("colors",), ("colors", "shapes", "shadows")):
        # warm-up (allocations, code objects), and the routes give the same results
        ra = run("grouped", feats)
        same = True
        for other in routes[1:]:
            rb = run(other, feats)
            same = same and all(
                a.n_unique == b.n_unique and a.compactness == b.compactness and np.array_equal(a.counts, b.counts)
                and np.array_equal(a.centers_rgb, b.centers_rgb) and a.shapes == b.shapes
                and a.n_contours == b.n_contours and (a.shadow_sum, a.shadow_count) == (b.shadow_sum, b.shadow_count)
                for a, b in zip(ra, rb))
        del ra, rb
        if not same:
            raise SystemExit(f"{feats}: the routes disagree")
        legs = {r: [] for r in routes}
        for _ in range(args.legs):
            for r in routes:
                legs[r].append(round(leg(r, feats), 1))
        med = {r: statistics.median(legs[r]) for r in routes}
        spread = max(legs["grouped"]) - min(legs["grouped"])
        # the base of the shapes pass is the best route without it, in this run: colours one pass
        base_spread = max(legs["one_pass"]) - min(legs["one_pass"])
        prof = {r: profiled(r, feats) for r in routes}
        out["features"]["+".join(feats)] = {
            "same_results": same, "images_per_s": legs, "median": med, "grouped_spread": round(spread, 1),
            "one_pass_over_grouped": round(med["one_pass"] / med["grouped"], 3),
            # the rule of DESIGN.md §3: a difference counts beyond three times the grouped legs' spread
            "difference_counts": abs(med["one_pass"] - med["grouped"]) > 3 * spread,
            "one_pass_spread": round(base_spread, 1),
            "both_over_one_pass": round(med["both"] / med["one_pass"], 3),
            "both_difference_counts": abs(med["both"] - med["one_pass"]) > 3 * base_spread,
            "colour_kernels_per_pass": {r: prof[r][0] for r in routes},
            "shape_kernels_per_pass": {r: prof[r][1] for r in routes},
            "host_contours_per_pass": {r: prof[r][2] for r in routes},
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
