#!/usr/bin/env python3
"""Resource table of one asm.sh output folder: per kernel (and pp_cubes) of kmeans.s / kmeans_wide.s the
figures of -Rpass-analysis=kernel-resource-usage and the instruction count of the function's body.

    python profiles/km_variants_retired/resources.py <label> <outdir>
"""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def main():
    label, out = sys.argv[1], sys.argv[2]
    for build, stem in (("narrow", "kmeans"), ("wide", "kmeans_wide")):
        res, cur = {}, None
        for line in open(f"{out}/{stem}.remarks"):
            m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
            if not m:
                continue
            if m.group(1):
                cur = res.setdefault(m.group(1), {})
            elif cur is not None:
                cur[m.group(2).strip()] = int(m.group(3))
        insts, fn = {}, None
        for line in open(f"{out}/{stem}.s"):
            m = re.match(r"(_Z\w+):", line)
            if m:
                fn = m.group(1)
                insts[fn] = 0
            elif line.startswith(".Lfunc_end"):
                fn = None
            elif fn and re.match(r"\t[a-z]", line):
                insts[fn] += 1
        # pp_cubes is a function, not a kernel: its figures are the "Function info" comments of the raw assembly,
        # its spills the "Folded Spill" / "Folded Reload" instructions of its body
        raw = open(f"{out}/{stem}.raw.s").read()
        m = re.search(r"\n(_ZN4llfe12_GLOBAL__N_18pp_cubes\w+):.*?\n\.Lfunc_end\d+:.*?; Function info:\n(.*?)\n\t\.text", raw, re.S)
        body, info = m.group(0), dict(re.findall(r"; (\w+): (\d+)", m.group(2)))
        print(f"{label} {build} pp_cubes VGPRs {info['NumVgprs']} SGPRs {info['TotalNumSgprs']} spill stores"
              f" {body.count('Folded Spill')} reloads {body.count('Folded Reload')} scratch {info['ScratchSize']}"
              f" insts {insts[m.group(1)]}")
        dm = demangle(list(res))
        for f, r in res.items():
            name = re.sub(r"\(.*", "", dm[f].replace("void ", "").replace("llfe::(anonymous namespace)::", ""))
            if not name.startswith(("k_kmeans<", "pp_cubes")):
                continue
            print(f"{label} {build} {name.replace(' ', '')} VGPRs {r['VGPRs']} SGPRs {r['TotalSGPRs']} SGPRspill {r['SGPRs Spill']}"
                  f" VGPRspill {r['VGPRs Spill']} scratch {r['ScratchSize']} LDS {r['LDS Size']} occ {r['Occupancy']}"
                  f" insts {insts.get(f, -1)}")


if __name__ == "__main__":
    main()
