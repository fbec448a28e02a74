"""The lane-role words of csrc/bc7_roles.h against the formulas they replaced, on the CPU.

A stand-alone host program includes bc7_roles.h, builds the table the kernel reads and indexes it the way the kernel
does: `role_rows32`, the macros that form a lane's address (R_ROW, R_WORDS, over L_H, L_HL, L_SLOT_OK, H_ALPHA) and the
line that forms the first gather source s1 are cut out of bc7_encode.hip as they stand.  (The kernel's Lowest instance
keeps its roles as expressions; the header describes its layout all the same and is checked for it here.)  For every
level, `pair` true and false, every stream trip the level walks, alpha-carrying and opaque halves, halves that walk the
second pass and halves that do not, and every lane of the wave it prints the two words and s1.  The test derives every field again from the per-lane formulas the encoder used before the words existed
(R_M6, R_VECP, R_SCA, R_CID, R_SLOT, R_SUB, R_PLANE, R_MI, R_RANK, R_IDBASE, the if / else-if ladder before the fit,
s2, use1, use2, leader) -- transcribed here in Python -- and compares.

Where the words deliberately say less than the formulas did, the test says so:
  * a lane that fits no subset has rank CF_ROLE_NO_RANK: the formulas gave such lanes a rank too, and phase 1 then left
    a partition in a register nobody read;
  * the words hold rank and mi, not the slot: the slot of the formulas must equal rank + mi * (slots of the first mode);
  * s1 is lane + 1 in every layout and is not stored: the kernel's own expression is compared;
  * s2 is compared on the lanes that use it, the leaders with use2: elsewhere the gathered values are discarded;
  * a lane without a role is inactive, and the channel set of a fit that does not run is not compared."""
import collections
import itertools
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
#include "bc7_roles.h"
#define __device__
#define __forceinline__ inline
static constexpr cf_bc7_role_table k_bc7_roles = cf_bc7_make_roles();
%(rows32)s
template <bool WIDE, int LEVEL>
static void walk(bool pair, uint32_t st, uint32_t a0, uint32_t a1, uint32_t g0, uint32_t g1)
{
	constexpr bool lay32 = !WIDE;
	constexpr uint32_t quality = WIDE ? 3u : (LEVEL == 1 ? 2u : (uint32_t)LEVEL);
	constexpr uint32_t rlay = WIDE ? CF_ROLE_LAY_WIDE : (quality == 2u ? CF_ROLE_LAY_NORMAL : CF_ROLE_LAY_LOWEST);
	const unsigned long long abal = (a0 ? 0x0400ull : 0ull) | (a1 ? 0x0002ull << 32 : 0ull);
	const unsigned long long gb = (g0 ? 1ull : 0ull) | (g1 ? 1ull << 32 : 0ull);
	for (uint32_t lane = 0; lane < 64u; ++lane) {
%(macros)s
		const uint32_t rw = R_WORDS[0], fw = R_WORDS[1];
		%(s1)s
		printf("%%d %%d %%u %%u %%u %%u %%u %%u %%u %%u %%u\n", LEVEL, (int)pair, st, a0, a1, g0, g1, lane, rw, fw, s1);
%(undefs)s
	}
}
int main()
{
	for (int pair = 0; pair < 2; ++pair)
		for (uint32_t st = 0; st < 2u; ++st)
			for (uint32_t m = 0; m < 16u; ++m) {
				const uint32_t a0 = m & 1u, a1 = (m >> 1) & 1u, g0 = (m >> 2) & 1u, g1 = (m >> 3) & 1u;
				if (st == 0u) { walk<false, 0>(pair, st, a0, a1, g0, g1); walk<false, 1>(pair, st, a0, a1, g0, g1); }
				walk<false, 2>(pair, st, a0, a1, g0, g1);
				// the wide layout holds one block per wave, and only an opaque block has a second pass
				if (!pair && (st == 0u || !a0)) { walk<true, 3>(pair, st, a0, a1, g0, g1); walk<true, 4>(pair, st, a0, a1, g0, g1); }
			}
	return 0;
}
"""

M6, VECP, SCA, PLANE = 1, 2, 4, 8
NO_RANK = 31
U32 = 0xFFFFFFFF


def _cut(text, start, end):
    a = text.find(start)
    assert a >= 0, "bc7_encode.hip no longer has the line %r" % start
    b = text.find(end, a)
    assert b >= 0, "bc7_encode.hip no longer has %r after %r" % (end, start)
    return text[a:b]


@pytest.fixture(scope="module")
def words(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    hip = open(os.path.join(CSRC, "bc7_encode.hip")).read()
    rows32 = _cut(hip, "__device__ __forceinline__ uint32_t role_rows32(", "// Encode one block with the whole wavefront")
    names = ("L_H", "L_HL", "L_SLOT_OK", "H_ALPHA", "R_ROW", "R_WORDS")
    macros = "\n".join(re.search(r"^#define %s .*$" % n, hip, re.M).group(0) for n in names)
    undefs = "\n".join("#undef %s" % n for n in names)
    s1 = re.search(r"^\s*const uint32_t s1 = .*;$", hip, re.M).group(0).strip()
    d = tmp_path_factory.mktemp("roles")
    src = d / "roles.cpp"
    src.write_text(PROGRAM % {"rows32": rows32, "macros": macros, "undefs": undefs, "s1": s1})
    exe = d / "roles"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return [tuple(int(v) for v in line.split()) for line in run.stdout.split("\n") if line.split()]


def formulas(level, pair, st, alpha, gate, lane, unitw, other_walks):
    """The roles of one lane by the encoder's earlier per-lane expressions.  alpha / gate: of the lane's own half;
    other_walks: some other half of the wave is opaque and walks the second pass (phase 1 then runs for the wave)."""
    wide = level >= 3
    quality = 3 if wide else (2 if level == 1 else level)
    lay32 = not wide
    hl = (lane & 31) if lay32 else lane
    hbase = (lane & 32) if pair else 0
    slot_ok = (not lay32) or pair or lane < 32
    s1l = lay32 and st == 1
    parts = quality >= 1 and ((not s1l) or (slot_ok and (not alpha) and gate) or other_walks)
    pfirst = (10 if quality == 2 else 4) if lay32 else (0 if st == 1 else 26)
    nslots = (11 if quality == 2 else 14) if lay32 else (10 if st == 1 else 16)
    ns = 2 + st
    nper0 = 5 if st == 1 else (((11 if alpha else 6) if quality == 2 else 14) if lay32 else (16 if alpha else 12))
    rel = (hl - pfirst) & U32
    if s1l:
        slot = hl if hl < 10 else ((hl - 11) & U32) >> 1
        sub = 2 if hl < 10 else ((hl - 11) & U32) & 1
    else:
        slot = rel // 3 if st == 1 else rel >> 1
        sub = (rel - slot*ns) & U32
    if s1l:
        plane = parts and slot_ok and (not alpha) and gate and hl != 10 and hl != 31
    else:
        plane = parts and slot_ok and hl >= pfirst and slot < nslots
    s1m4 = s1l and slot_ok and alpha and gate and 11 <= hl < 27
    mi = 1 if slot >= nper0 else 0
    rank = (slot - mi*nper0) & U32
    m6 = st == 0 and slot_ok and hl < 2
    if lay32:
        if st == 1:
            vecp = s1m4 and ((hl - 11) & 1) == 0
            sca = s1m4 and ((hl - 11) & 1) != 0
        elif quality == 2:
            vecp = slot_ok and 2 <= hl < 6
            sca = slot_ok and 6 <= hl < 10
        else:
            vecp = slot_ok and hl == 2
            sca = slot_ok and hl == 3
    else:
        vecp = st == 0 and 2 <= lane < 14
        sca = st == 0 and 14 <= lane < 26
    if m6:
        cid = 0
    elif lay32:
        cid = (5 + (((hl - 11) & U32) >> 1)) if st == 1 else ((hl - (5 if sca else 1)) if quality == 2 else 1)
    else:
        cid = 1 + (lane - (14 if sca else 2))
    idbase = ((256 if mi else 192) if st == 1 else (320 if alpha else (128 if mi else 64))) if plane else 0
    s2off = (4 if (quality == 2 and st == 0) else 1) if lay32 else (12 if st == 0 else 2)
    # the ladder before the fit
    rot, cb, ab, pbk, ib = 0, 7, 7, 1, 4
    active = m6
    if vecp or sca:
        if cid <= 4:
            rot, pbk, ib = cid - 1, 0, 2
            cb, ab = (0, 8) if sca else (7, 0)
            active = quality >= 2 or ((cid == 1) if quality == 1 else (cid == 1 and alpha))
            active = active and (unitw or rot == 0)
        else:
            isel = (cid - 5) >> 2
            rot, pbk = (cid - 5) & 3, 0
            cb, ab = (0, 6) if sca else (5, 0)
            ib = 2 if (isel != 0) == sca else 3
            active = quality >= 2 and (unitw or rot == 0)
    elif plane:
        mode = (2 if mi else 0) if st == 1 else (7 if alpha else (3 if mi else 1))
        cb, ab, pbk, ib = {1: (6, 0, 2, 3), 3: (7, 0, 1, 2), 0: (4, 0, 1, 3), 2: (5, 0, 0, 2)}.get(mode, (5, 5, 1, 2))
        active = True
    chm = 15 if m6 else (8 if sca else (7 if vecp else (15 if alpha else 7)))
    # after the fit
    tag_id = 0 if m6 else (cid if (vecp or sca) else idbase)      # + mypart on a subset lane
    tag_kf = 1 if sca else (sub if plane else 0)
    s1 = (lane + 1) & 63
    s2 = ((hbase + (((hl - 11) & U32) >> 1)) & 63) if (s1l and plane) else (lane + s2off) & 63
    use1 = plane
    use2 = vecp or (plane and st == 1)
    leader = active and ((hl == 0) if m6 else (vecp or (plane and sub == 0)))
    return dict(m6=m6, vecp=vecp, sca=sca, plane=plane, cid=cid, idbase=idbase, slot=slot, nper0=nper0, sub=sub, mi=mi, rank=rank, rot=rot,
                cb=cb, ab=ab, pbk=pbk, ib=ib, chm=chm, active=active, tag_id=tag_id, tag_kf=tag_kf, s1=s1, s2=s2, use1=use1,
                use2=use2, leader=leader, slot_ok=slot_ok, hl=hl, hbase=hbase)


def unpack(rw, fw):
    geo = (fw >> 2) & 0xFFFF
    return dict(kind=rw & 15, idb=(rw >> 4) & 511, kf=(rw >> 13) & 3, mi=(rw >> 15) & 1, rank=(rw >> 16) & 31,
                leader=(rw >> 21) & 1, use1=(rw >> 22) & 1, use2=(rw >> 23) & 1, s2=(rw >> 24) & 63,
                active_u=(rw >> 30) & 1, active_p=(rw >> 31) & 1,
                rot=fw & 3, cb=geo & 15, ab=(geo >> 4) & 15, pbk=(geo >> 8) & 15, ib=geo >> 12, chm=(fw >> 18) & 15)


def test_every_field_equals_the_per_lane_formulas(words):
    cases = words
    assert len(cases) > 5000
    seen = set()
    for level, pair, st, a0, a1, g0, g1, lane, rw, fw, s1 in cases:
        assert s1 == (lane + 1) & 63
        upper = bool(pair) and lane >= 32
        alpha, gate = bool(a1 if upper else a0), bool(g1 if upper else g0)
        oa, og = (a0, g0) if upper else (a1, g1)
        other_walks = bool(pair) and not oa and bool(og)
        w = unpack(rw, fw)
        lay = 2 if level >= 3 else (1 if level in (1, 2) else 0)
        for unitw in (True, False):
            f = formulas(level, bool(pair), st, alpha, gate, lane, unitw, other_walks)
            where = (level, pair, st, a0, a1, g0, g1, lane, unitw)
            kind = (M6 if f["m6"] else 0) | (VECP if f["vecp"] else 0) | (SCA if f["sca"] else 0) | (PLANE if f["plane"] else 0)
            assert kind in (0, M6, VECP, SCA, PLANE), where
            assert w["kind"] == kind, where
            assert (w["active_u"] if unitw else w["active_p"]) == int(f["active"]), where
            assert (w["leader"] & (w["active_u"] if unitw else w["active_p"])) == int(f["leader"]), where
            assert w["use1"] == int(f["use1"]) and w["use2"] == int(f["use2"]), where
            if kind == 0:
                assert not f["active"], where
                assert w["rank"] == NO_RANK and w["idb"] == 0 and w["kf"] == 0, where
                assert (w["rot"], w["cb"], w["ab"], w["pbk"], w["ib"]) == (f["rot"], f["cb"], f["ab"], f["pbk"], f["ib"]), where
                continue
            seen.add((lay, st, kind))
            # the geometry tag's inputs, the candidate id / id base, the fit index
            assert w["idb"] == f["tag_id"] and w["kf"] == f["tag_kf"], where
            if kind == PLANE:
                assert w["idb"] == f["idbase"] and w["kf"] == f["sub"], where
                assert w["mi"] == f["mi"] and w["rank"] == f["rank"], where
                assert w["rank"] + w["mi"]*f["nper0"] == f["slot"], where
            else:
                assert w["idb"] == f["cid"] and w["rank"] == NO_RANK, where
            if f["leader"] and f["use2"]:
                assert (f["hbase"] if lay != 2 else 0) + w["s2"] == f["s2"], where
            assert (w["rot"], w["cb"], w["ab"], w["pbk"], w["ib"], w["chm"]) == \
                (f["rot"], f["cb"], f["ab"], f["pbk"], f["ib"], f["chm"]), where
    # every kind of every layout and trip was reached
    want = {(0, 0, M6), (0, 0, VECP), (0, 0, SCA)}
    for lay in (1, 2):
        want |= {(lay, 0, k) for k in (M6, VECP, SCA, PLANE)} | {(lay, 1, PLANE)}
    want |= {(1, 1, VECP), (1, 1, SCA)}
    assert seen == want, sorted(seen ^ want)


def test_leaders_and_their_gather_sources(words):
    cases = words
    groups = itertools.groupby(cases, key=lambda c: c[:7])
    for key, lanes in groups:
        level, pair = key[0], key[1]
        width = 64 if level >= 3 else 32
        ws = {c[7]: unpack(c[8], c[9]) for c in lanes}
        assert len(ws) == 64
        for half in ((0, 32) if width == 32 else (0,)):
            mine = {l - half: ws[l] for l in range(half, half + width)}
            if width == 32 and half == 32 and not pair:
                assert all(w["kind"] == 0 for w in mine.values()), key
                continue
            cand = lambda w: (w["idb"], w["mi"], w["rank"])
            used = collections.Counter()
            leaders = [hl for hl, w in mine.items() if w["leader"]]
            # a candidate has one leader
            assert len({cand(mine[hl]) for hl in leaders}) == len(leaders), key
            for hl in leaders:
                w = mine[hl]
                assert w["kf"] == 0 and w["kind"] in (M6, VECP, PLANE), (key, hl)
                if w["use1"]:
                    assert hl + 1 < width, (key, hl)               # lane + 1 stays in the half
                    s = mine[hl + 1]
                    assert s["kind"] == PLANE and cand(s) == cand(w) and s["kf"] == 1, (key, hl)
                    assert (s["active_u"], s["active_p"]) == (w["active_u"], w["active_p"]), (key, hl)
                    used[hl + 1] += 1
                if w["use2"]:
                    assert w["s2"] < width, (key, hl)
                    s = mine[w["s2"]]
                    assert cand(s) == cand(w), (key, hl)
                    assert (s["kind"], s["kf"]) == ((SCA, 1) if w["kind"] == VECP else (PLANE, 2)), (key, hl)
                    assert (s["active_u"], s["active_p"]) == (w["active_u"], w["active_p"]), (key, hl)
                    used[w["s2"]] += 1
            # every lane that runs a fit is a leader or the source of exactly one (mode 6's second lane: its palette half)
            for hl, w in mine.items():
                if w["active_u"] and not w["leader"] and w["kind"] != M6:
                    assert used[hl] == 1, (key, hl)
                assert used[hl] <= 1 and not (w["leader"] and used[hl]), (key, hl)
