"""Compare two -Rpass-analysis=kernel-resource-usage dumps kernel by kernel, by mangled name.

    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Rpass-analysis=kernel-resource-usage -c FILE.hip -o /dev/null 2> dump.txt
    python tools/compare_resource_usage.py --parent parent_dump.txt [...] --this this_dump.txt [...] > report.txt

Prints, for every kernel both trees have, whether its registers, occupancy, scratch, spills and LDS size are equal (and what
changed where they are not), then the kernels only this tree has with their figures.  Exit status 1 when a kernel both trees have
differs in occupancy, LDS size, scratch or spills.  No GPU is needed.
"""
from __future__ import annotations

import argparse
import re
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
MUST_MATCH = ["ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def parse(paths):
    """{mangled name: {field: int}} of the dumps; a kernel that several files instantiate must agree with itself."""
    out = {}
    for p in paths:
        cur = None
        for line in open(p):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = {}
                out.setdefault(m.group(1), cur)
                continue
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
            if m and cur is not None and m.group(1) in FIELDS:
                cur[m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--this", nargs="+", required=True, dest="this")
    a = ap.parse_args()
    old, new = parse(a.parent), parse(a.this)
    bad = 0
    both = [k for k in new if k in old]
    print("# kernels in both trees: %d; only in this tree: %d; only in the parent: %d"
          % (len(both), len(new) - len(both), len([k for k in old if k not in new])))
    print("# -- kernels both trees have --")
    for k in both:
        diff = ["%s %d -> %d" % (f, old[k].get(f, -1), new[k].get(f, -1)) for f in FIELDS if old[k].get(f) != new[k].get(f)]
        hard = any(old[k].get(f) != new[k].get(f) for f in MUST_MATCH)
        bad += hard
        print("%s %s%s" % ("DIFFERS" if hard else ("equal  " if not diff else "regs   "), k, (": " + ", ".join(diff)) if diff else ""))
    for k in old:
        if k not in new:
            print("MISSING %s" % k)
            bad += 1
    print("# -- kernels only this tree has --")
    for k in new:
        if k not in old:
            print("new     %s: %s" % (k, ", ".join("%s %d" % (f, new[k].get(f, -1)) for f in FIELDS)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
