"""Memory check of the ragged header parse and of the entropy decode's host twin over tight slots,
CPU only: tools/jpeg_parse_images_check.cpp (its own main) and csrc/jpeg_decode.cpp (with
csrc/jpeg_huff_core.h, the decoding the kernels of csrc/jpeg_huff.hip compile) are built with
AddressSanitizer and UndefinedBehaviorSanitizer into one stand-alone program (the sanitizer
runtimes linked statically, so the program needs nothing of its environment).  It takes every case
of tests/jpeg_restate.py, the phase-locked and seam inputs, restart files and a set of malformed
files, whatever their sizes, as one ragged batch: llfe_jpeg_records_layout,
llfe_jpeg_parse_images into one exactly sized heap staging buffer and
llfe_jpeg_entropy_reference_images into exactly sized heap slots, compared with
llfe_jpeg_read_coefs_images.  No sanitizer is loaded into Python."""
import os
import subprocess

import numpy as np

from low_level_feature_extraction_amd import synth
from tests import jpeg_huff_cases as H
from tests import jpeg_restart_cases as RC
from tests import jpeg_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files(tmp_path):
    files = []

    def put(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        files.append(str(p))

    for i, (h, w, k) in enumerate(R.CASES):
        put(f"case{i:03d}.jpg", R.blob(h, w, k))
    for sub in (2, 1, 0):
        put(f"flat{sub}.jpg", H.flat(sub, False))
        put(f"stripe{sub}.jpg", H.flat(sub, True))
    put("boundary.jpg", H.stuffed_boundary()[0])
    for t in (H.SUB - 1, H.SUB, H.SUB + 1, 2 * H.SUB, 2 * H.SUB + 1):
        put(f"len{t}.jpg", H.scan_of_length(t))
    plain = sum(k in H.ACCEPTED for _, _, k in R.CASES) + 6 + 1 + 5
    restart = sum(k == 10 for _, _, k in R.CASES)
    for name, group in RC.cases().items():
        for j, b in enumerate(group):
            put(f"rst_{name}_{j}.jpg", b)
            restart += 1
    good = R.blob(240, 321, 0)
    rng = np.random.default_rng(8)
    malformed = {"flipped.jpg": H.flipped(good), "cut.jpg": H.cut(good), "cut1.jpg": H.cut(good, 1),
                 "truncated.jpg": good[:len(good) // 2] + b"\xff\xd9", "no_eoi.jpg": good[:len(good) // 2],
                 "header_only.jpg": good[:40], "not_a_jpeg.png": synth.encode_png(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)),
                 "empty.jpg": b""}
    noise = bytearray(good)  # the second half of the scan replaced by noise without FF bytes
    begin, end = H._scan_span(good)
    noise[(begin + end) // 2:end] = rng.integers(0, 255, end - (begin + end) // 2, dtype=np.uint8).tobytes()
    malformed["noise.jpg"] = bytes(noise)
    src = RC.damaged_source()
    for f in RC.DAMAGES:
        malformed[f"rst_{f.__name__}.jpg"] = f(src)
    for name, data in malformed.items():
        put(name, data)
    return files, plain, restart


def test_ragged_parse_and_reference_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "jpeg_parse_images_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "jpeg_parse_images_check.cpp"),
                    os.path.join(ROOT, "low_level_feature_extraction_amd", "csrc", "jpeg_decode.cpp"),
                    "-o", str(exe), "-ldl", "-lpthread"], check=True)
    files, plain, restart = _files(tmp_path)
    for flags, accepted in (([], plain), (["--restarts"], plain + restart)):
        r = subprocess.run([str(exe)] + flags + files, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "ok" and "ERROR" not in r.stderr and "runtime error" not in r.stderr
        # every eligible file decoded to the slot libjpeg extracts, and nothing else was accepted
        # unless it is a valid file of another image (a flip the code absorbs)
        assert sum(" equal 1" in ln for ln in lines if "flipped.jpg" not in ln) == accepted
        assert not any(" equal 0" in ln for ln in lines)
        for name in ("cut.jpg", "truncated.jpg", "noise.jpg"):
            assert any(name in ln and " parse 0 " in ln and " decode -5 / -5 " in ln for ln in lines), name
        if flags:
            for f in RC.DAMAGES:
                assert any(f"rst_{f.__name__}.jpg" in ln and " decode -5 / -5 " in ln for ln in lines), f.__name__
