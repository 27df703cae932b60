"""Memory check of the coefficient extraction, CPU only: tools/jpeg_coefs_check.cpp (its own
main) and csrc/jpeg_decode.cpp are compiled with AddressSanitizer and
UndefinedBehaviorSanitizer into one stand-alone program (the sanitizer runtimes linked
statically, so the program needs nothing of its environment), which extracts every case of
tests/jpeg_restate.py, and the files the path hands back, into exactly sized heap slots.
No sanitizer is loaded into Python."""
import io
import os
import subprocess

import numpy as np
from PIL import Image

from low_level_feature_extraction_amd import synth
from tests import jpeg_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extraction_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "jpeg_coefs_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "jpeg_coefs_check.cpp"),
                    os.path.join(ROOT, "low_level_feature_extraction_amd", "csrc", "jpeg_decode.cpp"),
                    "-o", str(exe), "-ldl", "-lpthread"], check=True)
    files = []

    def put(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        files.append(str(p))

    for i, (h, w, k) in enumerate(R.CASES):
        put(f"case{i:03d}.jpg", R.blob(h, w, k))
    rng = np.random.default_rng(8)
    arr = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    good = R.jpeg(arr, quality=90)
    cmyk = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (20, 30, 4), dtype=np.uint8), "CMYK").save(cmyk, "JPEG")
    put("cmyk.jpg", cmyk.getvalue())
    put("truncated.jpg", good[:len(good) // 2] + b"\xff\xd9")
    put("header_only.jpg", good[:40])
    bad = bytearray(good)
    sof = bytes(bad).index(b"\xff\xc0")
    bad[sof + 7:sof + 9] = b"\x00\x00"
    put("width0.jpg", bytes(bad))
    put("not_a_jpeg.png", synth.encode_png(arr))
    put("empty.jpg", b"")
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert sum(" status 0 " in ln for ln in lines) == len(R.CASES)  # every case extracted, nothing else
