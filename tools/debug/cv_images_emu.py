#!/usr/bin/env python
"""Builds tools/debug/cv_images_emu.cpp with -fsanitize=address,undefined (g++, C++20) and runs the
k_cv_images_* kernels on the host over the cases of tests/preprocess_images_cases.py, three kinds
of source (packed, row-strided, 3 bytes into its allocation), comparing with the oracle.  Needs no
GPU; libllfe.so must be built (it supplies cv_resize_plan).  An argument filters the case ids."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "low_level_feature_extraction_amd")
OUT = tempfile.mkdtemp(prefix="cv_images_emu_")
EMU, IN, RES = (os.path.join(OUT, f) for f in ("emu", "in.bin", "out.bin"))
subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{PKG}/csrc",
                f"-I{ROOT}/include", os.path.join(ROOT, "tools", "debug", "cv_images_emu.cpp"), "-o", EMU, f"-L{PKG}",
                "-lllfe", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"],
               check=True)
from tests import preprocess_images_cases as PC
from tests import resize_cases as RC

CODE = {"linear": 1, "area": 3, "lanczos4": 4}
cases = []
for k, c in enumerate(PC.seam_cases(64, 16)):
    cases.append((c.id, c.h, c.w, c.oh, c.ow, c.interp, k))
for m in PC.MODES:
    for k, c in enumerate(PC.rule_cases(m)):
        if c.resized and c.h * c.w < 200000:
            cases.append((c.id, c.h, c.w, c.oh, c.ow, c.interp, k))
for c in PC.stage_cases():
    cases.append((c.id, c.h, c.w, c.oh, c.ow, c.interp, 0))
cases.append(("copy", 37, 53, 37, 53, "area", 1))
only = sys.argv[1] if len(sys.argv) > 1 else None
bad = 0
for n, (cid, h, w, oh, ow, interp, k) in enumerate(cases):
    if only and only not in cid:
        continue
    x = np.asarray(PC.image(h, w, k))
    exp = PC.expected(h, w, oh, ow, interp, k)
    x.tofile(IN)
    kind = n % 3
    r = subprocess.run([EMU, str(h), str(w), str(oh), str(ow), str(CODE[interp]), str(kind),
                        IN, RES], capture_output=True, text=True)
    if r.returncode != 0:
        print("FAIL", cid, "rc", r.returncode, r.stdout[-300:], r.stderr[-1500:])
        bad += 1
        continue
    got = np.fromfile(RES, np.uint8).reshape(oh, ow, 3)
    ok = np.array_equal(got, exp)
    print("ok  " if ok else "DIFF", cid, "src", kind, r.stdout.strip(), "" if ok else int((got != exp).sum()))
    bad += not ok
print("bad:", bad)
sys.exit(1 if bad else 0)
