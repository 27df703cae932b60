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

``--pipeline`` measures fonts as a feature of the batched pipeline instead, on one resident
N x H x W ``synth`` batch (default 512 x 1080p), the two ways alternating, each timed
between device synchronisations, ``--reps`` (>= 5) times after ``--warmup`` runs of each:

  (a) the stage call beside the pipeline: process(batch, ("colors",)) then font_detect(batch)
  (b) the feature:                        process(batch, ("colors", "fonts"))
      (and once more per round with set_concurrency(False): the same kernels in order on one
      stream, which tells what the overlap with the colour stream is worth)
  (c) the front-end kernels alone, from llfe_kernel_stats with the streams serialised
      (set_concurrency(False)): k_font_binary + k_font_pack (font_detect) against
      k_font_bits (process(batch, ("fonts",))), with the other kernels of the font pass

and reports median and min-max of each, and whether (b) < (a) and k_font_bits < the pair
by more than the slower side's own min-max spread.  Prints one JSON line.

    python tools/bench_fonts.py --pipeline [--n 512] [--reps 7] [--warmup 2]
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


def _summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "spread": round(max(v) - min(v), 4), "runs": [round(x, 4) for x in v]}


def _pipeline(a):
    import torch

    from low_level_feature_extraction_amd import synth
    from low_level_feature_extraction_amd.backend import Backend

    reps = max(5, a.reps)
    n = a.n if a.n != 64 else 512
    batch = synth.synth_batch(n, a.height, a.width, seed=a.seed, device="cuda:0")
    be = Backend.get()
    FIELDS = ("n_contours", "n_regions", "x", "y", "width", "height", "gray_sum")

    def way_a():
        be.process(batch, ("colors",), seed=a.seed, index_base=0)
        return be.font_detect(batch)

    def way_b():
        return [r.font for r in be.process(batch, ("colors", "fonts"), seed=a.seed, index_base=0)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(max(1, a.warmup)):
        ra, rb = way_a(), way_b()
    same = all(x[f] == y[f] for x, y in zip(ra, rb) for f in FIELDS)
    ta, tb, ts = [], [], []
    for _ in range(reps):  # alternating
        ta.append(timed(way_a)[0])
        tb.append(timed(way_b)[0])
        be.set_concurrency(False)  # (b) with every kernel in order on one stream: no overlap
        try:
            ts.append(timed(way_b)[0])
        finally:
            be.set_concurrency(True)

    # (c) isolated kernel times: one stream, event-timed; every rep its own statistics
    be.set_concurrency(False)
    pair, bits, others = [], [], {}
    try:
        for _ in range(reps):
            be.set_profiling(True)
            be.font_detect(batch)
            torch.cuda.synchronize()
            st = be.kernel_stats()
            pair.append(st["k_font_binary"]["total_ms"] + st["k_font_pack"]["total_ms"])
            be.set_profiling(True)
            be.process(batch, ("fonts",))
            torch.cuda.synchronize()
            st = be.kernel_stats()
            bits.append(st["k_font_bits"]["total_ms"])
            for k, v in st.items():
                others.setdefault(k, []).append(v["total_ms"])
    finally:
        be.set_profiling(False)
        be.set_concurrency(True)
    A, B, P, K = _summary(ta), _summary(tb), _summary(pair), _summary(bits)
    out = {"tool": "bench_fonts --pipeline", "n": n, "height": a.height, "width": a.width, "reps": reps,
           "warmup": max(1, a.warmup), "records_equal": same, "found": sum(r["n_regions"] > 0 for r in rb),
           "a_colors_then_font_detect_ms": A, "b_colors_fonts_ms": B, "b_one_stream_ms": _summary(ts),
           "b_below_a_by_more_than_a_spread": A["median"] - B["median"] > A["spread"],
           "c_k_font_binary_plus_pack_ms": P, "c_k_font_bits_ms": K,
           "bits_below_pair_by_more_than_pair_spread": P["median"] - K["median"] > P["spread"],
           "c_font_pass_kernels_ms": {k: _summary(v) for k, v in sorted(others.items())}}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pipeline", action="store_true", help="fonts as a pipeline feature against the stage call")
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
    if a.pipeline:
        return _pipeline(a)
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
