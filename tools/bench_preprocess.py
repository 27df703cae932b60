#!/usr/bin/env python
"""Preprocessing (validate_and_preprocess_image's "auto" resize) of a batch of device-resident
images: the ragged call against the per-image route (DESIGN.md §3 "Preprocessing of a mixed-size
batch"; figures in profiles/preprocess_images/).  bench.py is not touched: this tool measures the
new entry point beside it.

  pair "resize"
    A  Backend.resize_cv per image at the rule's size: today's route (plan, table upload, launch
       and synchronisation per image)
    B  Backend.preprocess_images(feed, "auto"): one llfe_preprocess_images call
  pair "process"  process_images(feed, colors + shapes + shadows, preprocessing="auto",
                  colors="one_pass", shapes="one_pass")
    A  preprocess="per_image"
    B  preprocess="one_pass"

A seeded feed of --images images, then per pair one fresh process: a warm-up of both routes, then
A and B alternating for --legs legs each, every leg --reps passes over the feed; --runs such
processes per pair.  Every measuring process runs under --step-timeout seconds and nothing is
started after one that failed.
  --feed mixed    the 16 distinct sizes between 2000 x 1500 and 4032 x 3024 (w x h) of bench_thumb
  --feed uniform  every image 3840 x 2160 (w x h)
  --feed fast2x   every image 4000 x 3000 (w x h): exactly 2 x 2, the AREA_FAST kernel
After the timed legs of "resize" one profiled pass of each route gives the per-kernel ms
(llfe_kernel_stats), the kernels' ms per source megapixel and the host plan time of B.  One JSON
line per measuring process on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.bench_thumb import feed_sizes as thumb_feed_sizes  # noqa: E402

FEATURES = ("colors", "shapes", "shadows")


def feed_sizes(kind: str, n: int, seed: int):
    """(h, w) per image."""
    if kind == "fast2x":
        return [(3000, 4000)] * n
    return thumb_feed_sizes(kind, n, seed)


def measure(args):
    import torch

    from low_level_feature_extraction_amd.backend import Backend, preprocess_size

    be = Backend.get(0)
    sizes = feed_sizes(args.feed, args.images, args.seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    feed = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=g) for h, w in sizes]
    plans = [preprocess_size(w, h, "auto") for h, w in sizes]

    if args.pair == "resize":
        def route_a():
            return [be.resize_cv(t, p[0], p[1], p[2]) if p else t for t, p in zip(feed, plans)]

        def route_b():
            return be.preprocess_images(feed, "auto")

        ra, rb = route_a(), route_b()
        same = all(torch.equal(a, b) for a, b in zip(ra, rb))
        del ra, rb
    else:
        def run(preprocess):
            return be.process_images(feed, FEATURES, seed=0, index_base=0, preprocessing="auto", colors="one_pass",
                                     shapes="one_pass", preprocess=preprocess)

        def route_a():
            return run("per_image")

        def route_b():
            return run("one_pass")

        ra, rb = route_a(), route_b()
        same = all(x.n_unique == y.n_unique and x.palette == y.palette and x.shapes == y.shapes and
                   x.shadow_level == y.shadow_level and (x.width, x.height) == (y.width, y.height)
                   for x, y in zip(ra, rb))
        del ra, rb

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return args.reps * len(feed) / (time.perf_counter() - t0)

    legs = {"A": [], "B": []}
    for _ in range(args.legs):
        legs["A"].append(round(leg(route_a), 1))
        legs["B"].append(round(leg(route_b), 1))
    med = {k: float(np.median(v)) for k, v in legs.items()}
    spread_a = max(legs["A"]) - min(legs["A"])
    out = {
        "tool": "bench_preprocess", "pair": args.pair, "feed": args.feed, "images": len(feed),
        "distinct_sizes": len(set(sizes)), "resized": sum(p is not None for p in plans), "reps_per_leg": args.reps,
        "same_results": same, "images_per_s": legs, "median": med, "spread_A": round(spread_a, 1),
        # the project's rule: a gain is claimed where the medians differ by more than 3 x the base legs' spread
        "gain_claimed": bool(med["B"] - med["A"] > 3 * spread_a),
        "device": torch.cuda.get_device_name(0),
    }
    if args.pair == "resize":
        def profiled(fn):
            be.set_profiling(True)
            try:
                fn()
                st = be.kernel_stats()
            finally:
                be.set_profiling(False)
            return {k: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for k, v in st.items()}

        kb = profiled(route_b)
        mp = sum(h * w for (h, w), p in zip(sizes, plans) if p) / 1e6
        out["kernels_ms_per_pass_B"] = {k: v for k, v in kb.items() if k != "cv_images_plan_host"}
        out["host_plan_ms_per_pass_B"] = kb.get("cv_images_plan_host", {}).get("ms")
        out["source_megapixels_resized"] = round(mp, 2)
        out["kernel_ms_per_source_megapixel_B"] = {
            k: round(v["ms"] / mp, 5) for k, v in kb.items() if k in ("k_cv_images_area", "k_cv_images_area_fast")}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feed", choices=("mixed", "uniform", "fast2x"), default="mixed")
    ap.add_argument("--pair", choices=("resize", "process", "both"), default="both")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one measuring process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.legs < 3:
        ap.error("--legs: at least three legs each")
    if args.child:
        return measure(args)
    # the parent never opens the GPU: one fresh process per (run, pair), each under its own time
    # limit, and nothing after a failure
    pairs = ("resize", "process") if args.pair == "both" else (args.pair,)
    for run in range(args.runs):
        for pair in pairs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--feed", args.feed, "--pair", pair,
                   "--images", str(args.images), "--legs", str(args.legs), "--reps", str(args.reps),
                   "--seed", str(args.seed)]
            try:
                rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps({"tool": "bench_preprocess", "pair": pair, "feed": args.feed, "run": run,
                                  "failed": rc}), flush=True)
                sys.exit(1)


if __name__ == "__main__":
    main()
