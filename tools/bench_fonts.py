#!/usr/bin/env python3
"""Throughput of FontDetector.detect_font_batch on one GPU (not bench.py's flagship leg).

Calls only the public FontDetector.detect_font_batch, so the same file runs unchanged on
an older tree: copy it there and compare.  Inputs: N synthetic 1080p images, half ``ui``,
half ``photo`` (synth.synth_batch), once as a host array and once as a device tensor (a
tree that does not take a tensor reports that leg as null).  Each leg: warm-up batches,
then the wall time of every timed batch, ended by a device synchronise.  A digest of the
returned features lets two trees' answers be compared.  Where the tree has
Backend.font_detect, one more batch runs with event profiling on and the per-kernel
times of llfe_kernel_stats are printed (a run of its own: profiling is off in the timed
batches).  Prints one JSON line.

    python tools/bench_fonts.py [--n 64] [--height 1080] [--width 1920] [--reps 5] [--warmup 1]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _digest(feats) -> str:
    rows = [None if f is None else (f.font_family, f.font_size, f.font_style, f.confidence) for f in feats]
    return hashlib.sha256(repr(rows).encode()).hexdigest()[:16]


def _leg(torch, FontDetector, batch, reps, warmup):
    for _ in range(warmup):
        feats = FontDetector.detect_font_batch(batch)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        feats = FontDetector.detect_font_batch(batch)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    n = len(feats)
    med = statistics.median(times)
    return {"batch_s": [round(t, 5) for t in times], "median_s": round(med, 5), "min_s": round(min(times), 5),
            "max_s": round(max(times), 5), "images_per_s": round(n / med, 2),
            "found": sum(f is not None for f in feats), "digest": _digest(feats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--legs", default="host,device")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_fonts.py needs a GPU")
    from low_level_feature_extraction_amd import FontDetector, synth
    from low_level_feature_extraction_amd.backend import Backend

    dev = synth.synth_batch(a.n, a.height, a.width, seed=a.seed, device="cuda:0")
    host = dev.cpu().numpy()
    out = {"tool": "bench_fonts", "n": a.n, "height": a.height, "width": a.width, "reps": a.reps, "warmup": a.warmup,
           "device_path": hasattr(Backend, "font_detect"), "host_array": None, "device_tensor": None, "kernels": None}
    if "host" in a.legs:
        out["host_array"] = _leg(torch, FontDetector, host, a.reps, a.warmup)
    if "device" in a.legs:
        try:
            out["device_tensor"] = _leg(torch, FontDetector, dev, a.reps, a.warmup)
        except TypeError as e:  # a tree whose detect_font_batch converts its input with numpy
            out["device_tensor_error"] = str(e)[:120]
    if out["device_path"]:
        be = Backend.get()
        be.set_profiling(True)
        FontDetector.detect_font_batch(dev)
        torch.cuda.synchronize()
        stats = be.kernel_stats()
        be.set_profiling(False)
        out["kernels"] = {k: {"launches": v["launches"], "ms": round(v["total_ms"], 3)} for k, v in stats.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
