#!/usr/bin/env python
"""JPEG reconstruction on the device against the host decoder (DESIGN.md §3 "JPEG
reconstruction on the device"; figures in profiles/jpeg_recon/README.md).  bench.py and its
JPEG leg are not touched: this tool measures the opt-in path beside them.

  --host   CPU only, no GPU needed.  ms per 1080p quality-85 4:2:0 synth image per thread of
           A = llfe_decode_batch (entropy decode + reconstruction on the host) and
           B = llfe_jpeg_read_coefs_batch (entropy decode + coefficient copy), at 1 and at
           16 threads, five alternating runs each: median and min-max.  B / A is the share
           of a host decode that stays on the host.
  --gpu    MI355X.  bench.py's e2e serving loop (512 x 1080p, two batches in flight, three
           pinned staging buffers, a producer thread one batch ahead) with the producer
           A = decode.decode_batch into pinned BGR, submitted as a host batch, or
           B = decode.stage_coefs into pinned coefficient slots, then
               decode.reconstruct_staged (H2D + llfe_jpeg_reconstruct) and the device batch
               submitted, or
           C = decode.stage_bytes (headers parsed, scan bytes into pinned records), then
               decode.decode_staged_bytes (H2D of the records, llfe_jpeg_entropy_decode,
               llfe_jpeg_reconstruct) and the device batch submitted.
           A, B and C alternate in one process, --legs each; then the producers alone, the
           isolated kernel times (llfe_kernel_stats; llfe_jpeg_reconstruct reports its one
           launch as k_jpeg_images) and the H2D times of one batch of
           coefficients and of one batch of records.  The bar B had to clear over A is applied
           to C over B: every C leg above every B leg, medians further apart than three times
           B's min-max range.
           --restart-rows N encodes the feed with a restart marker every N MCU rows; leg C then
           stages with restarts=True (without it such files are refused by stage_bytes and C
           runs at B's speed plus a header parse).  Figures: profiles/jpeg_restart/.
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
    i, h, w, seed, restart_rows = args
    import io

    from PIL import Image

    from low_level_feature_extraction_amd import synth

    b = io.BytesIO()
    Image.fromarray(synth.synth_numpy(i, h, w, seed=seed)[:, :, ::-1]).save(
        b, "JPEG", quality=85, **({"restart_marker_rows": restart_rows} if restart_rows else {}))
    return b.getvalue()


def _blobs(n, h, w, seed, distinct=8, restart_rows=0):
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=distinct) as ex:
        d = list(ex.map(_encode, [(i, h, w, seed, restart_rows) for i in range(distinct)]))
    return [d[i % distinct] for i in range(n)]


def _spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "runs": len(v)}


def host(args):
    from low_level_feature_extraction_amd import _lib, decode

    h, w = args.height, args.width
    out = {"mode": "host", "image": f"{w}x{h} quality-85 4:2:0 synth", "codecs": decode.decoder_info(),
           "usable_cores": decode.usable_cores(), "unit": "ms per image per thread"}
    for threads in (1, 16):
        n = args.host_images * threads
        blobs = _blobs(n, h, w, args.seed)
        bgr = np.empty((n, h, w, 3), np.uint8)
        st = decode.stage_coefs(blobs[:1], 1)
        stride = (st.used_bytes + 127) // 128 * 128
        slots = np.empty((n, stride), np.uint8)
        descs = (_lib.LlfeJpegDesc * n)()

        def a():
            assert not any(decode._native(blobs, h, w, bgr, threads))

        def b():
            assert not any(decode._read_coefs(blobs, h, w, slots, descs, threads))

        a(), b()  # warm: pages touched, library loaded
        ta, tb = [], []
        for _ in range(args.runs):
            for fn, acc in ((a, ta), (b, tb)):
                t = time.perf_counter()
                fn()
                acc.append((time.perf_counter() - t) * 1e3 * threads / n)
        out[f"threads_{threads}"] = {"images_per_run": n, "A_decode_batch": _spread(ta), "B_read_coefs": _spread(tb),
                                     "B_over_A_medians": round(statistics.median(tb) / statistics.median(ta), 3)}
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
    blobs = _blobs(B, h, w, args.seed, restart_rows=args.restart_rows)
    restarts = args.restart_rows > 0
    pinned = [torch.empty((B, h, w, 3), dtype=torch.uint8).pin_memory() for _ in range(3)]
    bufs = [p.numpy() for p in pinned]
    outs = [torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    st0 = decode.stage_coefs(blobs[:2], threads)
    slot_bytes = (st0.used_bytes + 127) // 128 * 128  # a 4:2:0 feed: half of the 4:4:4 slot
    side = torch.cuda.Stream()
    # the two paths give the same bytes (checked once, on the first images)
    with torch.cuda.stream(side):
        dev = decode.decode_batch_device(blobs[:4], workers=threads)
    assert np.array_equal(dev.cpu().numpy(), decode.decode_batch(blobs[:4], workers=threads))
    be.process(bufs[0][:2], feats, seed=args.seed)

    def leg(kind):
        def produce(k):
            if kind == "A":
                return decode.decode_batch(blobs, bufs[k % 3], threads)
            if kind == "C":
                return decode.stage_bytes(blobs, threads, slot_bytes=slot_bytes, restarts=restarts)
            return decode.stage_coefs(blobs, threads, slot_bytes=slot_bytes)

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
                        item = decode.reconstruct_staged(item, 0, threads, out=outs[k % 3])
                elif kind == "C":
                    with torch.cuda.stream(side):
                        item = decode.decode_staged_bytes(item, 0, threads, out=outs[k % 3])
                pending.append(be.submit(item, feats, seed=args.seed + k))
                if len(pending) == 2:
                    be.collect(pending.pop(0))
            while pending:
                be.collect(pending.pop(0))
            return B * steps / (time.perf_counter() - t0)

    with torch.cuda.stream(side):
        dev = decode.decode_batch_device(blobs[:4], workers=threads, entropy="device", restarts=restarts)
    assert np.array_equal(dev.cpu().numpy(), decode.decode_batch(blobs[:4], workers=threads))
    leg("A"), leg("B"), leg("C")  # warm all three: pinned rings, workspaces, thread pools
    va, vb, vc = [], [], []
    for _ in range(args.legs):
        va.append(leg("A"))
        vb.append(leg("B"))
        vc.append(leg("C"))
    # producers alone, warm: what bounds each leg from the host side
    t = time.perf_counter()
    decode.decode_batch(blobs, bufs[0], threads)
    prod_a = time.perf_counter() - t
    t = time.perf_counter()
    st = decode.stage_coefs(blobs, threads, slot_bytes=slot_bytes)
    prod_b = time.perf_counter() - t
    t = time.perf_counter()
    sb = decode.stage_bytes(blobs, threads, slot_bytes=slot_bytes, restarts=restarts)
    prod_c = time.perf_counter() - t
    assert sb.status == [0] * B
    # H2D of one batch of coefficients, and the kernels alone
    d_slots = torch.empty((B, slot_bytes), dtype=torch.uint8, device="cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    h2d = []
    for _ in range(3):
        e0.record()
        d_slots.copy_(st.tensor, non_blocking=True)
        e1.record()
        e1.synchronize()
        h2d.append(e0.elapsed_time(e1))
    be.set_profiling(True)
    for _ in range(3):
        be.jpeg_reconstruct(d_slots, st.descs, h, w, out=outs[0])
    ks = be.kernel_stats()
    be.set_profiling(False)
    kern = {k: {"ms": round(v["total_ms"] / 3, 3), "launches": v["launches"] // 3,
                "GB_per_s": round(v["bytes"] / max(v["total_ms"], 1e-9) / 1e6, 1)}
            for k, v in ks.items() if k.startswith("k_jpeg")}
    # the same for leg C: H2D of one batch of records (what the file is long, row by row), the
    # entropy kernels alone, and how many images they took
    used = sb.used_bytes
    d_rec = torch.empty((B, sb.records.shape[1]), dtype=torch.uint8, device="cuda:0")
    h2d_c = []
    for _ in range(3):
        e0.record()
        for i in range(B):
            d_rec[i, :used].copy_(sb.tensor[i, :used], non_blocking=True)
        e1.record()
        e1.synchronize()
        h2d_c.append(e0.elapsed_time(e1))
    be.set_profiling(True)
    for _ in range(3):
        taken = be.jpeg_entropy_decode(d_rec, sb.scans, sb.descs, h, w, d_slots)
    ks = be.kernel_stats()
    be.set_profiling(False)
    kern_c = {k: {"ms": round(v["total_ms"] / 3, 3), "launches": v["launches"] // 3}
              for k, v in ks.items() if k.startswith("k_huff")}
    scan_total = sum(s_.scan_bytes for s_ in sb.scans)
    a, b, c = _spread(va), _spread(vb), _spread(vc)
    bar = min(vb) > max(va) and (b["median"] - a["median"]) > 3 * (a["max"] - a["min"])
    bar_c = min(vc) > max(vb) and (c["median"] - b["median"]) > 3 * (b["max"] - b["min"])
    print(json.dumps({
        "mode": "gpu", "unit": "images/s", "batch": B, "image": f"{w}x{h} quality-85 4:2:0 synth", "steps_per_leg": steps,
        "restart_rows": args.restart_rows, "restart_interval_mcus": sb.scans[0].restart_interval,
        "decode_threads": threads, "features": list(feats), "A_decode_batch": a, "B_coefficients": b,
        "C_device_entropy": c,
        "A_legs": [round(v, 1) for v in va], "B_legs": [round(v, 1) for v in vb], "C_legs": [round(v, 1) for v in vc],
        "B_over_A_medians": round(b["median"] / a["median"], 3), "bar_met": bool(bar),
        "C_over_B_medians": round(c["median"] / b["median"], 3), "C_bar_met": bool(bar_c),
        "producer_alone_ms_per_batch": {"A_decode_batch": round(prod_a * 1e3, 1), "B_stage_coefs": round(prod_b * 1e3, 1),
                                        "C_stage_bytes": round(prod_c * 1e3, 1)},
        "slot_bytes": slot_bytes, "coef_MiB_per_batch": round(B * slot_bytes / 2**20, 1),
        "h2d_ms_per_batch": _spread(h2d), "kernel_ms_per_batch": kern,
        "C_record_MiB_per_batch": round(B * used / 2**20, 1), "C_scan_MiB_per_batch": round(scan_total / 2**20, 1),
        "C_subsequences_per_image_max": max(-(-s_.scan_bytes // 128) for s_ in sb.scans),
        "C_h2d_ms_per_batch": _spread(h2d_c), "C_kernel_ms_per_batch": kern_c,
        "C_images_taken_by_device": sum(1 for rc in taken if rc == 0)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=6, help="batches per leg (--gpu)")
    ap.add_argument("--legs", type=int, default=4, help="legs of each producer, alternating (--gpu)")
    ap.add_argument("--runs", type=int, default=5, help="alternating runs (--host)")
    ap.add_argument("--host-images", type=int, default=16, help="images per thread and run (--host)")
    ap.add_argument("--restart-rows", type=int, default=0,
                    help="encode the feed with a restart marker every N MCU rows; leg C stages with restarts=True (--gpu)")
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
