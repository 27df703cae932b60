#!/usr/bin/env python
"""PNG decode on the device against the host decoder (DESIGN.md §3 "PNG decode on the device";
figures in profiles/png_inflate/README.md).  bench.py and its PNG leg are not touched: this tool
measures the opt-in path beside them.

  --host   CPU only, no GPU needed.  ms per 1080p synth PNG per thread of
           A = llfe_decode_batch (inflate + unfilter + BGR on the host) and
           B = llfe_png_parse_batch (chunk walk, CRCs, the deflate stream copied into a record),
           at 1 and at 16 threads, alternating runs: median and min-max.  B / A is the share of
           a host decode that stays on the host.
  --gpu    MI355X.  bench.py's e2e serving loop (512 x 1080p synth images as Pillow writes them,
           50 / 50 ui / photo, two batches in flight, three pinned staging buffers, a producer
           thread one batch ahead) with the producer
           A = decode.decode_batch into pinned BGR, submitted as a host batch, or
           B = decode.stage_png into pinned records, then decode.decode_staged_png (H2D of the
               records, llfe_png_decode_device) and the device batch submitted.
           A and B alternate in one process, --legs each; then the producers alone, the H2D of
           one batch of records and the isolated kernel times (llfe_kernel_stats).
           --kind ui|photo encodes the feed from one synth class only.
One JSON line per mode on stdout.
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


def _encode(args):
    i, h, w, seed, kind = args
    from low_level_feature_extraction_amd import synth

    return synth.encode_png(synth.synth_numpy(i, h, w, seed=seed, kind=kind))


def _blobs(n, h, w, seed, kind=None, distinct=8):
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=distinct) as ex:
        d = list(ex.map(_encode, [(i, h, w, seed, kind) for i in range(distinct)]))
    return [d[i % distinct] for i in range(n)]


def _spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "runs": len(v)}


def host(args):
    from low_level_feature_extraction_amd import decode

    h, w = args.height, args.width
    out = {"mode": "host", "image": f"{w}x{h} synth PNG ({args.kind or 'ui/photo'})", "codecs": decode.decoder_info(),
           "usable_cores": decode.usable_cores(), "unit": "ms per image per thread"}
    for threads in (1, 16):
        n = args.host_images * threads
        blobs = _blobs(n, h, w, args.seed, args.kind)
        bgr = np.empty((n, h, w, 3), np.uint8)

        def a():
            assert not any(decode._native(blobs, h, w, bgr, threads))

        def b():
            assert not any(decode.stage_png(blobs, threads, size=(h, w)).status)

        a(), b(), b(), b()  # warm: pages touched, library loaded, the ring of three filled
        ta, tb = [], []
        for _ in range(args.runs):
            for fn, acc in ((a, ta), (b, tb)):
                t = time.perf_counter()
                fn()
                acc.append((time.perf_counter() - t) * 1e3 * threads / n)
        out[f"threads_{threads}"] = {"images_per_run": n, "A_decode_batch": _spread(ta), "B_stage_png": _spread(tb),
                                     "B_over_A_medians": round(statistics.median(tb) / statistics.median(ta), 4)}
    out["file_MB"] = _spread([len(b_) / 1e6 for b_ in blobs[:8]])
    print(json.dumps(out))


def gpu(args):
    from concurrent.futures import ThreadPoolExecutor

    import torch

    from low_level_feature_extraction_amd import decode
    from low_level_feature_extraction_amd.backend import Backend

    B, h, w, steps = args.batch, args.height, args.width, args.steps
    feats = tuple(args.features.split(","))
    be = Backend.get(0)
    threads = decode.default_decode_threads()
    blobs = _blobs(B, h, w, args.seed, args.kind)
    pinned = [torch.empty((B, h, w, 3), dtype=torch.uint8).pin_memory() for _ in range(3)]
    bufs = [p.numpy() for p in pinned]
    outs = [torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    side = torch.cuda.Stream()
    # the two paths give the same bytes (checked once, on the first images)
    with torch.cuda.stream(side):
        dev = decode.decode_batch_device(blobs[:8], workers=threads, png="device")
    assert np.array_equal(dev.cpu().numpy(), decode.decode_batch(blobs[:8], workers=threads))
    be.process(bufs[0][:2], feats, seed=args.seed)

    def leg(kind):
        def produce(k):
            if kind == "A":
                return decode.decode_batch(blobs, bufs[k % 3], threads)
            return decode.stage_png(blobs, threads, size=(h, w))

        with ThreadPoolExecutor(max_workers=1) as prod:
            t0 = time.perf_counter()
            fut = prod.submit(produce, 0)
            pending = []
            for k in range(steps):
                item = fut.result()
                if k + 1 < steps:
                    fut = prod.submit(produce, k + 1)
                if kind == "B":
                    with torch.cuda.stream(side):
                        item = decode.decode_staged_png(item, 0, threads, out=outs[k % 3])
                pending.append(be.submit(item, feats, seed=args.seed + k))
                if len(pending) == 2:
                    be.collect(pending.pop(0))
            while pending:
                be.collect(pending.pop(0))
            return B * steps / (time.perf_counter() - t0)

    leg("A"), leg("B")  # warm both: pinned rings, workspaces, thread pools
    va, vb = [], []
    for _ in range(args.legs):
        va.append(leg("A"))
        vb.append(leg("B"))
    # producers alone, warm: what bounds each leg from the host side
    t = time.perf_counter()
    decode.decode_batch(blobs, bufs[0], threads)
    prod_a = time.perf_counter() - t
    t = time.perf_counter()
    sp = decode.stage_png(blobs, threads, size=(h, w))
    prod_b = time.perf_counter() - t
    assert sp.status == [0] * B
    # H2D of one batch of records (what the file is long, row by row), and the kernels alone
    used = sp.used_bytes
    d_rec = torch.empty((B, sp.records.shape[1]), dtype=torch.uint8, device="cuda:0")
    raw = torch.empty((B, sp.raw_stride), dtype=torch.uint8, device="cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    h2d = []
    for _ in range(3):
        e0.record()
        for i in range(B):
            d_rec[i, :used].copy_(sp.tensor[i, :used], non_blocking=True)
        e1.record()
        e1.synchronize()
        h2d.append(e0.elapsed_time(e1))
    be.set_profiling(True)
    for _ in range(3):
        taken = be.png_decode(d_rec, sp.descs, h, w, outs[0], raw)
    ks = be.kernel_stats()
    be.set_profiling(False)
    kern = {k: {"ms": round(v["total_ms"] / 3, 3), "launches": v["launches"] // 3}
            for k, v in ks.items() if k.startswith("k_png")}
    a, b = _spread(va), _spread(vb)
    print(json.dumps({
        "mode": "gpu", "unit": "images/s", "batch": B, "image": f"{w}x{h} synth PNG ({args.kind or 'ui/photo'})",
        "steps_per_leg": steps, "decode_threads": threads, "features": list(feats), "A_decode_batch": a,
        "B_device_png": b, "A_legs": [round(v, 1) for v in va], "B_legs": [round(v, 1) for v in vb],
        "B_over_A_medians": round(b["median"] / a["median"], 3),
        "B_every_leg_above_A": bool(min(vb) > max(va)),
        "producer_alone_ms_per_batch": {"A_decode_batch": round(prod_a * 1e3, 1), "B_stage_png": round(prod_b * 1e3, 1)},
        "file_MB": _spread([len(b_) / 1e6 for b_ in blobs[:8]]),
        "record_MiB_per_batch": round(B * used / 2**20, 1),
        "deflate_MiB_per_batch": round(sum(d.deflate_bytes for d in sp.descs) / 2**20, 1),
        "raw_MiB_per_batch": round(sum(d.raw_bytes for d in sp.descs) / 2**20, 1),
        "h2d_ms_per_batch": _spread(h2d), "kernel_ms_per_batch": kern,
        "images_taken_by_device": sum(1 for rc in taken if rc == 0)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=4, help="batches per leg (--gpu)")
    ap.add_argument("--legs", type=int, default=3, help="legs of each producer, alternating (--gpu)")
    ap.add_argument("--runs", type=int, default=5, help="alternating runs (--host)")
    ap.add_argument("--host-images", type=int, default=8, help="images per thread and run (--host)")
    ap.add_argument("--kind", choices=["ui", "photo"], default=None, help="one synth class instead of both")
    ap.add_argument("--features", default="colors,shapes,shadows")
    ap.add_argument("--seed", type=int, default=2025)
    args = ap.parse_args()
    if not (args.host or args.gpu):
        ap.error("pick --host and / or --gpu")
    if args.host:
        host(args)
    if args.gpu:
        gpu(args)


if __name__ == "__main__":
    main()
