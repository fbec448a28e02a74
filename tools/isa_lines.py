#!/usr/bin/env python3
"""Static VALU, scalar and branch instructions of one kernel instance per region of its source, from the line table
of the assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -gline-tables-only \
          --cuda-device-only -S -o bc7.s cuttlefish_amd/csrc/bc7_encode.hip
    python tools/isa_lines.py bc7.s cuttlefish_amd/csrc/bc7_encode.hip [--kernel MANGLED_SUBSTRING]

Inlined code keeps the line of the statement it came from, so a region is a range of source lines: from the first
line that contains its start text to the line before the one that contains its end text.  Lines of other files
(headers) are counted per file.  Instructions the compiler gives line 0 (merged or generated code: the rejoin of a
divergent branch, a hoisted constant) go to the region of the last source line before them.  Scalar instructions are
every s_* that is no branch (s_nop and s_waitcnt among them), branches every s_branch / s_cbranch_*.  The counts are
static: a region inlined at n call sites is counted n times, a loop body once per copy.  What runs how often is not
in this table.  A start or end text may be a tuple of alternatives: the first line that holds any of them (the same
region in sources that word its opening differently).

--classes prints another table: per region, how many of its VALU instructions are in the 2-cycle class and how many in
the 4-cycle class (the class list of tools/isa_mix.py), and how many v_mov_b32 and s_nop it holds; the last line gives
the v_mov_b32 the compiler put on line 0.
"""
import argparse
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import FAST  # noqa: E402

# (label, text that opens the region, text of the first line after it); searched in this order from the top
_ASSEMBLY = ("// the fit this lane's geometry-cache column now holds", "// ---- assemble candidates in their leader lanes")
_CAND_GEO = ("// The same geometry from what the candidate's leader stored with it",
             "// It is read from what the candidate's leader stored with it")
# (where the texel loop hands its error out: the unit-weight search forms it later, from the key sum)
_ERR_OUT = ("\tf.err = err;", "\tif (!UNITW) f.err = err;")
# (a fourth element marks a region that not every source has -- fit_geo left the encoder, cand_geo came late --: skipped
# where its opening is missing, so that this source and its parents can both be tabulated)
BC7_REGIONS = (
    ("quantize", "__device__ __forceinline__ void quantize(", "// View of one block's texels in LDS"),
    ("assign_lsq_lane: palette", "__device__ __forceinline__ void assign_lsq_lane(", ("\tuint32_t err = pp_sum;", "\tuint32_t err = UNITW ? 0u : pp_sum;")),
    ("assign_lsq_lane: texel loop", ("\tuint32_t err = pp_sum;", "\tuint32_t err = UNITW ? 0u : pp_sum;"), _ERR_OUT),
    ("assign_lsq_lane: refit sums", _ERR_OUT, "// Least squares WITH the quantisation inside"),
    ("refit_window", "__device__ __forceinline__ void refit_window(", "// Fit-geometry cache"),
    ("fit_lane", "__device__ __forceinline__ void fit_lane(", "__device__ __forceinline__ uint32_t w2i("),
    ("pack_block_group", "__device__ __forceinline__ uint4 pack_block_group(", "// The 14 integer moments of a set of texels"),
    ("fit_geo", "__device__ __forceinline__ FitGeo fit_geo(", _CAND_GEO + ("// Store a fit (quantised fields",), "optional"),
    ("cand_geo / geo_src", _CAND_GEO, "// Store a fit (quantised fields", "optional"),
    ("phase 1", "// ---- phase 1: partition scores", "// ---- lane roles ----"),
    ("lane roles before the fit", "// ---- lane roles ----", "\t\t\tuint32_t wl[4] = {wt[0], wt[1], wt[2], wt[3]};"),
    ("starts-trip epilogue", "// the roles below are computed again from here", _ASSEMBLY),
    ("candidate assembly", _ASSEMBLY, "#undef R_"),
    ("perturbation pass", "// ---- endpoint perturbation (oracle: uber_refine)", "\treturn pack_block_group("),
)


def is_valu(op):
    return op.startswith("v_") and not op.startswith(("v_readlane", "v_readfirstlane", "v_writelane"))


def is_branch(op):
    return op.startswith(("s_branch", "s_cbranch"))


def is_salu(op):
    return op.startswith("s_") and not is_branch(op)


def _find(src, text, at):
    texts = (text,) if isinstance(text, str) else text
    return next((i for i in range(at, len(src)) if any(t in src[i] for t in texts)), None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("source")
    ap.add_argument("--kernel", default="cfhip_bc7_encode_kernelILi0ELb1ELb0ELi2E")
    ap.add_argument("--classes", action="store_true", help="per region: VALU by issue class, v_mov_b32 and s_nop counts")
    a = ap.parse_args()
    src = open(a.source).read().split("\n")
    regions, at = [], 0
    for label, start, end, *optional in BC7_REGIONS:
        s = _find(src, start, at)
        if s is None and optional:
            continue
        if s is None:
            raise SystemExit("%s: no line with %r (region %r): update BC7_REGIONS" % (a.source, start, label))
        e = _find(src, end, s + 1)
        if e is None:
            raise SystemExit("%s: no line with %r after line %d (end of region %r): update BC7_REGIONS" % (a.source, end, s + 1, label))
        regions.append((label, s + 1, e))        # 1-based, inclusive
        at = s
    files, counts, ops = {}, collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
    cls = collections.defaultdict(collections.Counter)      # region -> fast / slow / mov / nop
    inside, cur, line0, mov_line0 = False, ("?", 0), False, 0
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
            line0 = int(m.group(2)) == 0
            if not line0:                     # line 0 stays with the source line before it
                cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        op = t.split()[0] if t and not t.startswith((".", ";")) and not t.endswith(":") else ""
        kind = "valu" if is_valu(op) else ("branch" if is_branch(op) else ("salu" if is_salu(op) else None))
        if kind is None:
            continue
        key = "other files: " + cur[0]
        if cur[0] == os.path.basename(a.source):
            key = next((lab for lab, s, e in regions if s <= cur[1] <= e), "rest of " + cur[0])
        counts[key][kind] += 1
        if kind == "valu":
            ops[key][op.replace("_e32", "").replace("_e64", "")] += 1
            plain = re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", op)
            cls[key]["fast" if plain in FAST else "slow"] += 1
            if plain == "v_mov_b32":
                cls[key]["mov"] += 1
                mov_line0 += line0
        elif op == "s_nop":
            cls[key]["nop"] += 1
    total = {k: sum(c[k] for c in counts.values()) for k in ("valu", "salu", "branch")}
    print("%s: %d static VALU instructions, %d scalar, %d branches" % (a.kernel, total["valu"], total["salu"], total["branch"]))
    print("  %-34s %5s  %6s  %5s %6s   %s" % ("region", "VALU", "", "SALU", "branch", "most frequent VALU"))
    for key, c in sorted(counts.items(), key=lambda kv: -kv[1]["valu"]):
        top = ", ".join("%s %d" % kv for kv in ops[key].most_common(6))
        print("  %-34s %5d  %4.1f %%  %5d  %5d   %s" % (key, c["valu"], 100.0*c["valu"]/max(total["valu"], 1), c["salu"], c["branch"], top))
    if a.classes:
        tot = collections.Counter()
        for c in cls.values():
            tot.update(c)
        print("  %-34s %7s %7s %9s %6s" % ("region", "2-cycle", "4-cycle", "v_mov_b32", "s_nop"))
        for key, c in sorted(cls.items(), key=lambda kv: -(kv[1]["fast"] + kv[1]["slow"])):
            print("  %-34s %7d %7d %9d %6d" % (key, c["fast"], c["slow"], c["mov"], c["nop"]))
        print("  %-34s %7d %7d %9d %6d   (%d of the v_mov_b32 on line 0)" % ("all", tot["fast"], tot["slow"], tot["mov"], tot["nop"], mov_line0))


if __name__ == "__main__":
    main()
