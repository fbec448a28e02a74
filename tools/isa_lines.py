#!/usr/bin/env python3
"""Static VALU instructions of one kernel instance per region of its source, from the line table of the assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -gline-tables-only \
          --cuda-device-only -S -o bc7.s cuttlefish_amd/csrc/bc7_encode.hip
    python tools/isa_lines.py bc7.s cuttlefish_amd/csrc/bc7_encode.hip [--kernel MANGLED_SUBSTRING]

Inlined code keeps the line of the statement it came from, so a region is a range of source lines: from the first
line that contains its start text to the line before the one that contains its end text.  Lines of other files
(headers) are counted per file.  The counts are static: a region inlined at n call sites is counted n times, a
loop body once per copy.  What runs how often is not in this table.
"""
import argparse
import collections
import os
import re

# (label, text that opens the region, text of the first line after it); searched in this order from the top
BC7_REGIONS = (
    ("quantize", "__device__ __forceinline__ void quantize(", "// View of one block's texels in LDS"),
    ("assign_lsq_lane: palette", "__device__ __forceinline__ void assign_lsq_lane(", "\tuint32_t err = pp_sum;"),
    ("assign_lsq_lane: texel loop", "\tuint32_t err = pp_sum;", "\tf.err = err;"),
    ("assign_lsq_lane: refit sums", "\tf.err = err;", "// Least squares WITH the quantisation inside"),
    ("refit_window", "__device__ __forceinline__ void refit_window(", "// Fit-geometry cache"),
    ("fit_lane", "__device__ __forceinline__ void fit_lane(", "__device__ __forceinline__ uint32_t w2i("),
)


def is_valu(op):
    return op.startswith("v_") and not op.startswith(("v_readlane", "v_readfirstlane", "v_writelane"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("source")
    ap.add_argument("--kernel", default="cfhip_bc7_encode_kernelILi0ELb1ELb0ELi2E")
    a = ap.parse_args()
    src = open(a.source).read().split("\n")
    regions, at = [], 0
    for label, start, end in BC7_REGIONS:
        s = next((i for i in range(at, len(src)) if start in src[i]), None)
        if s is None:
            raise SystemExit("%s: no line with %r (region %r): update BC7_REGIONS" % (a.source, start, label))
        e = next((i for i in range(s + 1, len(src)) if end in src[i]), None)
        if e is None:
            raise SystemExit("%s: no line with %r after line %d (end of region %r): update BC7_REGIONS" % (a.source, end, s + 1, label))
        regions.append((label, s + 1, e))        # 1-based, inclusive
        at = s
    files, counts, ops = {}, collections.Counter(), collections.defaultdict(collections.Counter)
    inside, cur = False, ("?", 0)
    for line in open(a.asm):
        t = line.strip()
        m = re.match(r'\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]+)"', t)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
            continue
        if re.match(r"_Z\w+:", t):
            inside = a.kernel in t
            continue
        if not inside:
            continue
        if t.startswith(".Lfunc_end"):
            inside = False
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        op = t.split()[0] if t and not t.startswith((".", ";")) and not t.endswith(":") else ""
        if not is_valu(op):
            continue
        key = "other files: " + cur[0]
        if cur[0] == os.path.basename(a.source):
            key = next((lab for lab, s, e in regions if s <= cur[1] <= e), "rest of " + cur[0])
        counts[key] += 1
        ops[key][op.replace("_e32", "").replace("_e64", "")] += 1
    total = sum(counts.values())
    print("%s: %d static VALU instructions" % (a.kernel, total))
    for key, n in sorted(counts.items(), key=lambda kv: -kv[1]):
        top = ", ".join("%s %d" % kv for kv in ops[key].most_common(6))
        print("  %-34s %5d  %4.1f %%   %s" % (key, n, 100.0*n/total, top))


if __name__ == "__main__":
    main()
