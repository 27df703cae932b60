"""The pair-table lookup of the two-centre cube split (csrc/kmeans_lattice.h, what the Lloyd kernel
compiles) against a plain restatement of the 64-step walk, CPU only: tools/km_lattice_check.cpp (its
own main) is built with AddressSanitizer and UndefinedBehaviorSanitizer into one stand-alone program
(the sanitizer runtimes linked statically) and run.  It compares the four sign words bit for bit, for
both orders of the pair: exhaustive steps in [-3, 3]^3 at every F0q within two units of the band's
edges at every position, the tie families (zero, equal, 512-multiple and tiny steps), more than 10^5
random step sets at full range, and arbitrary float32 centres (the reversed pair's steps are the
table's, negated).  No sanitizer is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lookup_equals_walk_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "km_lattice_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "low_level_feature_extraction_amd", "csrc"),
                    os.path.join(ROOT, "tools", "km_lattice_check.cpp"), "-o", str(exe), "-ldl", "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    fams = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in lines[:-1]}
    assert set(fams) == {"small", "ties", "tiny", "random", "float_centres", "pairs"}
    assert all(bad == 0 for _, bad in fams.values()), fams
    assert fams["small"][0] == 343 * 64 * 2 * 2 * 5 * 2
    assert fams["random"][0] >= 2 * 2 * 100000 and fams["pairs"][0] == 10
