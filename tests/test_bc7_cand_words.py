"""The candidate word of csrc/bc7_cand.h against the id ladder it replaced, on the CPU.

A stand-alone host program includes bc7_cand.h, builds the two tables the kernel reads (candidate words by shape, fit
masks by subset count, partition and fit) and, for every candidate id the encoder can produce -- 0 (mode 6), 1..12
(modes 5 and 4) and 64..383 (the partition modes) -- and every fit index 0..3, takes the fields of the fit the way the
kernel does: the word from the table entry of the id (what the leader stores into word 6 of its column, above the
p-bits), the fields by cf_bc7_cand_fit_of, the texels by the mask table.  The word it decodes carries p-bits, as the
stored word does.  The test derives every field again from `fit_geo`, the ladder bc7_encode.hip had before the word existed -- transcribed
here in Python, the only place it still stands -- and compares: mode, part, rot, isel, ns, nfits, cb, ab, pbk, ib, chm, mask, m6, planes45, sca.

It also runs column_put_fit's read-modify-write of the p-bit word -- the expression is cut out of bc7_encode.hip as it
stands -- on the stored word, for every fit slot and every value of the p-bits: the two new bits land, the other p-bits
and the candidate's fields stay."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuttlefish_amd", "csrc")

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "bc7_cand.h"
static constexpr cf_bc7_cand_table k_bc7_cands = cf_bc7_make_cands();
static constexpr cf_bc7_mask_table k_bc7_masks = cf_bc7_make_masks();
static void one(uint32_t id)
{
	const uint32_t cw = k_bc7_cands.w[cf_bc7_cand_index(id)];
	if (cw != cf_bc7_cand_word(id) || (cw & CF_CAND_PB_MASK) != 0u || cf_bc7_cand_index(id) >= CF_CAND_TABLE_N) {
		printf("bad word %u\n", id);
		return;
	}
	for (uint32_t kf = 0; kf < 4u; ++kf) {
		// the stored word holds the p-bits below the fields: all of them set must not reach a field
		const cf_bc7_cand_fit g = cf_bc7_cand_fit_of(cw | CF_CAND_PB_MASK, id, kf);
		if (g.mi >= sizeof(k_bc7_masks.m)/sizeof(k_bc7_masks.m[0])) { printf("bad index %u %u\n", id, kf); continue; }
		printf("F %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d %d %d\n", id, kf, g.mode, g.part, g.rot, g.isel, g.ns, g.nfits,
			g.cb, g.ab, g.pbk, g.ib, g.chm, (uint32_t)k_bc7_masks.m[g.mi], (int)g.m6, (int)g.planes45, (int)g.sca);
	}
	// column_put_fit's read-modify-write of word 6
	for (uint32_t kf = 0; kf < 3u; ++kf)
		for (uint32_t old = 0; old < 64u; ++old)
			for (uint32_t pb = 0; pb < 4u; ++pb) {
				const uint32_t pw = cw | old;
				const uint32_t nw = %(rmw)s;
				printf("W %%u %%u %%u %%u %%u %%u\n", id, kf, old, pb, cw, nw);
			}
}
int main()
{
	for (uint32_t id = 0; id < 13u; ++id) one(id);
	for (uint32_t id = 64u; id < 384u; ++id) one(id);
	// a word that is none (a column no leader stored into) must still index the mask table
	for (uint32_t w = 0; w < 4u; ++w)
		for (uint32_t kf = 0; kf < 4u; ++kf)
			printf("I %%u\n", cf_bc7_cand_fit_of(w << 12, 0x7FFFFFFFu, kf).mi);
	return 0;
}
"""

PART2 = [
    0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000,
    0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310, 0x3100, 0x8cce, 0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c,
    0xaaaa, 0xf0f0, 0x5a5a, 0x33cc, 0x3c3c, 0x55aa, 0x9696, 0xa55a, 0x73ce, 0x13c8, 0x324c, 0x3bdc, 0x6996, 0xc33c, 0x9966, 0x0660,
    0x0272, 0x04e4, 0x4e40, 0x2720, 0xc936, 0x936c, 0x39c6, 0x639c, 0x9336, 0x9cc6, 0x817e, 0xe718, 0xccf0, 0x0fcc, 0x7744, 0xee22]
PART3 = [
    0xaa685050, 0x6a5a5040, 0x5a5a4200, 0x5450a0a8, 0xa5a50000, 0xa0a05050, 0x5555a0a0, 0x5a5a5050,
    0xaa550000, 0xaa555500, 0xaaaa5500, 0x90909090, 0x94949494, 0xa4a4a4a4, 0xa9a59450, 0x2a0a4250,
    0xa5945040, 0x0a425054, 0xa5a5a500, 0x55a0a0a0, 0xa8a85454, 0x6a6a4040, 0xa4a45000, 0x1a1a0500,
    0x0050a4a4, 0xaaa59090, 0x14696914, 0x69691400, 0xa08585a0, 0xaa821414, 0x50a4a450, 0x6a5a0200,
    0xa9a58000, 0x5090a0a8, 0xa8a09050, 0x24242424, 0x00aa5500, 0x24924924, 0x24499224, 0x50a50a50,
    0x500aa550, 0xaaaa4444, 0x66660000, 0xa5a0a5a0, 0x50a050a0, 0x69286928, 0x44aaaa44, 0x66666600,
    0xaa444444, 0x54a854a8, 0x95809580, 0x96969600, 0xa85454a8, 0x80959580, 0xaa141414, 0x96960000,
    0xaaaa1414, 0xa05050a0, 0xa0a5a5a0, 0x96000000, 0x40804080, 0xa9a8a9a8, 0xaaaaaa44, 0x2a4a5254]


def part3_mask(p3, sb):
    """part3_mask of bc7_encode.hip: the texels whose two bits equal sb (none for sb = 3)"""
    lo, hi = p3 & 0x55555555, (p3 >> 1) & 0x55555555
    x = {0: ~(lo | hi) & 0x55555555, 1: lo & ~hi, 2: hi & ~lo}.get(sb, 0) & 0xFFFFFFFF
    x = (x | (x >> 1)) & 0x33333333
    x = (x | (x >> 2)) & 0x0F0F0F0F
    x = (x | (x >> 4)) & 0x00FF00FF
    return (x | (x >> 8)) & 0xFFFF


def nib(word, mode):
    return (word >> (4*mode)) & 15


def fit_geo(id_, kf):
    """fit_geo as bc7_encode.hip had it, line by line"""
    g = dict(part=0, rot=0, isel=0)
    if id_ == 0:
        g["mode"] = 6
    elif id_ < 5:
        g.update(mode=5, rot=id_ - 1)
    elif id_ < 13:
        g.update(mode=4, rot=(id_ - 5) & 3, isel=(id_ - 5) >> 2)
    elif id_ < 128:
        g.update(mode=1, part=id_ - 64)
    elif id_ < 192:
        g.update(mode=3, part=id_ - 128)
    elif id_ < 256:
        g.update(mode=0, part=id_ - 192)
    elif id_ < 320:
        g.update(mode=2, part=id_ - 256)
    else:
        g.update(mode=7, part=(id_ - 320) & 63)
    mode = g["mode"]
    g["ns"] = nib(0x21112323, mode)
    g["m6"] = mode == 6
    g["planes45"] = mode in (4, 5)
    g["nfits"] = 2 if g["planes45"] else g["ns"]
    g["sca"] = g["planes45"] and kf == 1
    g["mask"] = 0xFFFF
    if g["planes45"]:
        ibc = 2 if mode == 5 else (3 if g["isel"] else 2)
        iba = 2 if mode == 5 else (2 if g["isel"] else 3)
        g["cb"] = 0 if g["sca"] else (7 if mode == 5 else 5)
        g["ab"] = (8 if mode == 5 else 6) if g["sca"] else 0
        g["ib"] = iba if g["sca"] else ibc
        g["pbk"] = 0
        g["chm"] = 8 if g["sca"] else 7
    else:
        g["cb"], g["ab"] = nib(0x57757564, mode), nib(0x57860000, mode)
        g["pbk"], g["ib"] = nib(0x11001021, mode), nib(0x24222233, mode)
        g["chm"] = 15 if g["ab"] else 7
        if g["ns"] == 2:
            p2 = PART2[g["part"]]
            g["mask"] = p2 if kf else (~p2 & 0xFFFF)
        elif g["ns"] == 3:
            g["mask"] = part3_mask(PART3[g["part"]], kf)
    return g


FIELDS = ("mode", "part", "rot", "isel", "ns", "nfits", "cb", "ab", "pbk", "ib", "chm", "mask", "m6", "planes45", "sca")
IDS = [0] + list(range(1, 13)) + list(range(64, 384))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    hip = open(os.path.join(CSRC, "bc7_encode.hip")).read()
    m = re.search(r"^\s*wc\[6\*CF_WG_THREADS\] = (.*);$", hip, re.M)
    assert m, "bc7_encode.hip no longer has column_put_fit's store of word 6"
    d = tmp_path_factory.mktemp("cand")
    src = d / "cand.cpp"
    src.write_text(PROGRAM.replace("%(rmw)s", m.group(1)).replace("%%", "%"))
    exe = d / "cand"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    out = [line.split() for line in run.stdout.split("\n") if line.split()]
    assert not [l for l in out if l[0] == "bad"], [l for l in out if l[0] == "bad"][:5]
    return out


def test_every_field_equals_fit_geo(lines):
    seen = set()
    for rec in lines:
        if rec[0] != "F":
            continue
        v = [int(x) for x in rec[1:]]
        id_, kf = v[0], v[1]
        got = dict(zip(FIELDS, v[2:]))
        want = fit_geo(id_, kf)
        for f in FIELDS:
            assert got[f] == int(want[f]), (id_, kf, f, got[f], want[f])
        seen.add((id_, kf))
    assert seen == {(i, k) for i in IDS for k in range(4)}


def test_three_subset_words_have_no_fourth_subset():
    """A fit index past the subsets gets no texels: part3_mask answers 0 there, the table compares two bits with kf"""
    assert all(((p >> (2*t)) & 3) != 3 for p in PART3 for t in range(16))


def test_partition_tables_are_the_format_s(lines):
    """The header's tables (which the kernel's k_part2 / k_part3 are initialised from) through the masks of subset 1 / 2"""
    masks = {(int(r[1]), int(r[2])): int(r[14]) for r in lines if r[0] == "F"}
    for p in range(64):
        assert masks[(64 + p, 1)] == PART2[p] and masks[(320 + p, 0)] == (~PART2[p] & 0xFFFF)
        for sb in range(3):
            want = sum(1 << t for t in range(16) if ((PART3[p] >> (2*t)) & 3) == sb)
            assert masks[(192 + p, sb)] == masks[(256 + p, sb)] == want


def test_a_word_that_is_no_candidate_still_indexes_the_table(lines):
    idx = [int(r[1]) for r in lines if r[0] == "I"]
    assert len(idx) == 16 and all(0 <= i < 4*64*4 for i in idx)


def test_put_fit_keeps_the_word_and_the_other_pbits(lines):
    n = 0
    for rec in lines:
        if rec[0] != "W":
            continue
        id_, kf, old, pb, cw, nw = (int(x) for x in rec[1:])
        assert nw >> 6 == cw >> 6 and cw & 63 == 0, (id_, kf, old, pb)
        assert nw & 63 == (old & ~(3 << (2*kf))) | (pb << (2*kf)), (id_, kf, old, pb)
        n += 1
    assert n == len(IDS)*3*64*4
