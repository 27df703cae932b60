#!/usr/bin/env python
"""JPEG decode of a batch of uploads into device memory: the mixed-size device path against the
two routes there were before it (DESIGN.md §3 "JPEG decode of a mixed-size batch"; figures in
profiles/jpeg_images/).  bench.py is not touched: this tool measures the new entry point beside it.

  A  decode.decode_many (decode_bgr per image on the decode pool) and one upload per image:
     what ImageProcessor.auto_process_images(device=True) does by default
  B  group the feed by size, decode.decode_batch_device per group (llfe_jpeg_reconstruct: the
     kernel of C, one launch per group)
  C  decode.decode_images_device: one staging buffer, one launch (csrc/jpeg_images.hip)
  D  decode.decode_images_device(entropy="device"): C with the entropy decode on the device too
     (csrc/jpeg_huff.hip; DESIGN.md §3 "JPEG entropy decode of a mixed-size batch"; figures in
     profiles/jpeg_huff_images/), measured against C, the path it replaces

A seeded feed of --images quality-85 4:2:0 JPEGs, one process, one rank, a warm-up of all four
(which also compares their bytes), then A, B, C and D alternating for --legs legs each, every leg
--reps passes over the feed:
  --feed mixed    the 16 sizes of tools/bench_thumb.py --feed mixed (2000 x 1500 .. 4032 x 3024)
  --feed uniform  every image 1920 x 1080, where B is at its best
  --feed phone    the mixed feed, pixel for pixel, with the EXIF orientation of half the files set
                  to 6, of a quarter to 8 and of one to 3: a phone's portrait shots (DESIGN.md §3
                  "EXIF orientation in the mixed-size decode"; figures in profiles/jpeg_orient/).
                  Its legs are C and D as above (orient="host": those files take decode_bgr, the
                  behaviour before the option) against Co and Do, the same two with
                  orient="device"; A and B are not run.  The profiled passes give k_jpeg_images per
                  orientation group (k_jpeg_images, _mirrored, _transposed).
After the timed legs one profiled pass of C and of D gives the kernel ms (llfe_kernel_stats):
k_jpeg_images, and D's k_huff_* kernels (k_huff_sync: one launch per pass and kind).  One JSON
line on stdout.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def phone_orientation(i: int):
    """The EXIF orientation of file i of the phone feed (None: no EXIF): 6 for every second file,
    8 for every fourth, 3 for one."""
    return 6 if i % 2 == 0 else 8 if i % 4 == 1 else 3 if i == 3 else None


def make_feed(kind: str, n: int, seed: int):
    """-> (list of (h, w), list of JPEG blobs): smooth colour fields with some texture, so the
    files are of a photo's length rather than noise's.  (h, w) is the coded size."""
    from bench_thumb import feed_sizes
    from PIL import Image

    from concurrent.futures import ThreadPoolExecutor

    sizes = [(1080, 1920)] * n if kind == "uniform" else feed_sizes("mixed", n, seed)
    orient = phone_orientation if kind == "phone" else lambda i: None

    def one(i):
        h, w = sizes[i]
        rng = np.random.default_rng([seed, i])
        y, x = np.arange(h, dtype=np.float32)[:, None], np.arange(w, dtype=np.float32)[None, :]
        f = rng.uniform(0.002, 0.02, (3, 2)).astype(np.float32)
        img = np.stack([127 + 100 * np.sin(f[c, 0] * x + f[c, 1] * y + i + c) for c in range(3)], axis=-1)
        img += rng.normal(0, 6, (h, w, 1)).astype(np.float32)
        b = io.BytesIO()
        kw = {}
        if orient(i) is not None:
            ex = Image.Exif()
            ex[0x0112] = orient(i)
            kw["exif"] = ex.tobytes()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(b, "JPEG", quality=85, subsampling=2, **kw)
        return b.getvalue()

    with ThreadPoolExecutor(8) as pool:
        return sizes, list(pool.map(one, range(n)))


def run_legs(args, routes, n):
    """Every route alternating, --legs legs each -> {route: [images/s per leg]}."""
    import torch

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return args.reps * n / (time.perf_counter() - t0)

    legs = {k: [] for k in routes}
    for _ in range(args.legs):
        for k, fn in routes.items():
            legs[k].append(round(leg(fn), 1))
    return legs


def profiled(be, fn):
    be.set_profiling(True)
    try:
        fn()
        st = be.kernel_stats()
    finally:
        be.set_profiling(False)
    return {k: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for k, v in st.items()
            if k.startswith(("k_jpeg", "k_huff"))}


def phone(args, be, sizes, blobs, route_c, route_d):
    """The phone feed: orient="host" (C, D) against orient="device" (Co, Do)."""
    import torch

    from low_level_feature_extraction_amd import decode

    routes = {"C": route_c, "Co": lambda: decode.decode_images_device(blobs, orient="device"),
              "D": route_d, "Do": lambda: decode.decode_images_device(blobs, entropy="device", orient="device")}
    for _ in range(3):  # (the warm-up of main)
        res = [fn() for fn in routes.values()]
    same = all(all(torch.equal(r[0], x) for x in r[1:]) for r in zip(*res))
    del res
    legs = run_legs(args, routes, len(blobs))
    kernels = {k: profiled(be, fn) for k, fn in routes.items()}
    summary = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in legs.items()}
    spread = max(summary[k]["max"] - summary[k]["min"] for k in ("C", "D"))
    mp = {}
    for i, (h, w) in enumerate(sizes):
        o = phone_orientation(i) or 1
        mp[o] = mp.get(o, 0) + h * w / 1e6
    out = {
        "tool": "bench_jpeg_mixed", "feed": args.feed, "images": len(blobs), "distinct_sizes": len(set(sizes)),
        "megapixels": round(sum(h * w for h, w in sizes) / 1e6, 1), "file_mib": round(sum(map(len, blobs)) / 2**20, 1),
        "megapixels_by_orientation": {str(o): round(v, 1) for o, v in sorted(mp.items())},
        "reps_per_leg": args.reps, "same_bytes": same, "decode_threads": decode.default_decode_threads(),
        "images_per_s": legs, "summary": summary,
        # a speed claim needs the medians further apart than three times the host legs' spread
        "Co_minus_C_median": round(summary["Co"]["median"] - summary["C"]["median"], 1),
        "Do_minus_D_median": round(summary["Do"]["median"] - summary["D"]["median"], 1),
        "three_times_host_spread": round(3 * spread, 1),
        "kernels_ms_per_pass": kernels,
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feed", choices=("mixed", "uniform", "phone"), default="mixed")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.legs < 3:
        ap.error("--legs: at least three legs each")

    import torch

    from low_level_feature_extraction_amd import decode
    from low_level_feature_extraction_amd.backend import Backend

    if not torch.cuda.is_available():
        sys.exit("bench_jpeg_mixed: no GPU (this tool measures nothing without one)")
    be = Backend.get(0)
    sizes, blobs = make_feed(args.feed, args.images, args.seed)

    def route_a():
        return [torch.from_numpy(a).cuda() for a in decode.decode_many(blobs)]

    def route_b():
        groups: dict = {}
        for i, s in enumerate(sizes):
            groups.setdefault(s, []).append(i)
        out = [None] * len(blobs)
        for idx in groups.values():
            res = decode.decode_batch_device([blobs[i] for i in idx])
            for j, i in enumerate(idx):
                out[i] = res[j]
        return out

    def route_c():
        return decode.decode_images_device(blobs)

    def route_d():
        return decode.decode_images_device(blobs, entropy="device")

    routes = {"A": route_a, "B": route_b, "C": route_c, "D": route_d}
    if args.feed == "phone":
        return phone(args, be, sizes, blobs, route_c, route_d)
    # warm-up: three passes each, so that every buffer of the pinned staging rings of three exists
    # (allocations, code objects), and the four routes give the same bytes
    for _ in range(3):
        ra, rb, rc, rd = route_a(), route_b(), route_c(), route_d()
    same = all(torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) for a, b, c, d in zip(ra, rb, rc, rd))
    del ra, rb, rc, rd

    legs = run_legs(args, routes, len(blobs))
    kc, kd = profiled(be, route_c), profiled(be, route_d)
    summary = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in legs.items()}
    spread = max(summary[k]["max"] - summary[k]["min"] for k in ("A", "B"))
    out = {
        "tool": "bench_jpeg_mixed", "feed": args.feed, "images": len(blobs), "distinct_sizes": len(set(sizes)),
        "megapixels": round(sum(h * w for h, w in sizes) / 1e6, 1), "file_mib": round(sum(map(len, blobs)) / 2**20, 1),
        "reps_per_leg": args.reps, "same_bytes": same, "decode_threads": decode.default_decode_threads(),
        "images_per_s": legs, "summary": summary,
        # a speed claim needs the medians further apart than three times the base routes' spread
        "C_minus_best_base_median": round(summary["C"]["median"] - max(summary["A"]["median"], summary["B"]["median"]), 1),
        "D_minus_C_median": round(summary["D"]["median"] - summary["C"]["median"], 1),
        "three_times_base_spread": round(3 * spread, 1),
        "kernels_ms_per_pass": {"C": kc, "D": kd},
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
