#!/usr/bin/env python
"""Thumbnails of a batch of device-resident images: the ragged call against the size-grouped
route (DESIGN.md §3 "Thumbnails of a mixed-size batch"; figures in profiles/thumb_images/).
bench.py is not touched: this tool measures the new entry point beside it.

  A  group the feed by size, Backend.thumbnail_pil_batch(torch.stack(group)) per group: what
     ImageProcessor.auto_process_images does by default, given images already on the device
  B  Backend.thumbnail_pil_images(feed): one llfe_thumbnail_pil_images call

A seeded feed of --images images at the default box (1920, 1080), one process, a warm-up of
both, then A and B alternating for --legs legs each, every leg --reps passes over the feed:
  --feed mixed    16 distinct sizes between 2000 x 1500 and 4032 x 3024 (w x h)
  --feed uniform  every image 3840 x 2160 (w x h), where A is at its best
After the timed legs one profiled pass of each gives the per-kernel ms (llfe_kernel_stats) and
the host plan time of B.  One JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def feed_sizes(kind: str, n: int, seed: int):
    """(h, w) per image."""
    if kind == "uniform":
        return [(2160, 3840)] * n
    r = np.random.default_rng(seed)
    sizes = [(1500, 2000), (3024, 4032)]
    while len(sizes) < 16:
        s = (int(r.integers(1500, 3025)), int(r.integers(2000, 4033)))
        if s not in sizes:
            sizes.append(s)
    # every size at least once when the feed allows it, the rest drawn, in a seeded order
    idx = list(range(min(16, n))) + [int(i) for i in r.integers(0, 16, max(n - 16, 0))]
    return [sizes[i] for i in r.permutation(idx)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feed", choices=("mixed", "uniform"), default="mixed")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-w", type=int, default=1920)
    ap.add_argument("--max-h", type=int, default=1080)
    args = ap.parse_args()
    if args.legs < 3:
        ap.error("--legs: at least three legs each")

    import torch

    from low_level_feature_extraction_amd.backend import Backend

    be = Backend.get(0)
    sizes = feed_sizes(args.feed, args.images, args.seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    feed = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=g) for h, w in sizes]
    box = (args.max_w, args.max_h)

    def route_a():
        groups: dict = {}
        for i, t in enumerate(feed):
            groups.setdefault(tuple(t.shape), []).append(i)
        out = [None] * len(feed)
        for idx in groups.values():
            res = be.thumbnail_pil_batch(torch.stack([feed[i] for i in idx]), *box)
            for j, i in enumerate(idx):
                out[i] = res[j]
        return out

    def route_b():
        return be.thumbnail_pil_images(feed, *box)

    # warm-up (allocations, code objects), and the two routes give the same bytes
    ra, rb = route_a(), route_b()
    same = all(torch.equal(a, b) for a, b in zip(ra, rb))
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

    def profiled(fn):
        be.set_profiling(True)
        try:
            fn()
            st = be.kernel_stats()
        finally:
            be.set_profiling(False)
        return {k: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for k, v in st.items()}

    ka, kb = profiled(route_a), profiled(route_b)
    out = {
        "tool": "bench_thumb", "feed": args.feed, "images": len(feed), "distinct_sizes": len(set(sizes)),
        "box": list(box), "reps_per_leg": args.reps, "same_bytes": same,
        "images_per_s": legs, "B_slowest_over_A_fastest": round(min(legs["B"]) / max(legs["A"]), 3),
        "kernels_ms_per_pass": {"A": ka, "B": {k: v for k, v in kb.items() if k != "thumb_plan_host"}},
        "host_plan_ms_per_pass": kb.get("thumb_plan_host", {}).get("ms"),
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
