"""Memory check of the PNG staging and of the device decode's host twin, CPU only:
tools/png_inflate_check.cpp (its own main) and csrc/png_decode.cpp (with csrc/png_inflate_core.h,
the decoding the kernels of csrc/png_inflate.hip compile) are built with AddressSanitizer and
UndefinedBehaviorSanitizer into one stand-alone program (the sanitizer runtimes linked
statically, so the program needs nothing of its environment).  It stages every case and every
anomaly of tests/png_cases.py into exactly sized heap records and decodes them into exactly
sized raw and pixel buffers: a bit reader that left the staged stream, a match that reached
before the buffer or a store outside it is a sanitizer report.  No sanitizer is loaded into
Python."""
import os
import subprocess

from tests import png_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_and_reference_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "png_inflate_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "png_inflate_check.cpp"),
                    os.path.join(ROOT, "low_level_feature_extraction_amd", "csrc", "png_decode.cpp"),
                    "-o", str(exe), "-lz", "-ldl", "-lpthread"], check=True)
    files = []
    for i, c in enumerate(P.CASES):
        p = tmp_path / f"{i:03d}_{c['name']}.png"
        p.write_bytes(c["blob"])
        files.append(str(p))
    good = next(c for c in P.CASES if c["name"] == "level6")["blob"]
    for name, data in (("empty", b""), ("signature_only", good[:8]), ("header_only", good[:33]), ("half", good[:len(good) // 2])):
        p = tmp_path / f"zz_{name}.png"
        p.write_bytes(data)
        files.append(str(p))
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert len(lines) == len(files) + 1
    for c, ln in zip(P.CASES, lines):
        if c["kind"] == "ok":
            assert ln.endswith(" parse 0 decode 0 equal 1"), ln
        elif c["kind"] == "anomaly":
            assert ln.endswith(" parse 0 decode -5 equal -1"), ln
        elif c["name"] == "other_size":  # (parsed at its own size here: a good file)
            assert ln.endswith(" parse 0 decode 0 equal 1"), ln
        else:
            assert " parse -5 " in ln, ln
    for ln in lines[len(P.CASES):-1]:
        assert " parse 0 " not in ln, ln
