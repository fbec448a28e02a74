"""The integer statistics BC7's first stream trip hands to its fits (csrc/bc7_packed.h: mom_whole, mom_sub, mom_unpack,
byte_lohi) against plain per-texel sums, on the CPU.

A stand-alone host program includes csrc/bc7_packed.h as it stands.  For every block it builds the per-block table the
kernel's prologue builds (words 0..3 = q_cc | s_c << 20, words 4..9 = q01 q02 q03 q12 q13 q23, every alpha term zero
when the block is opaque) and the per-channel extremes, then checks
  whole-block fits: for rotations 0..3 x the vector (7) and scalar (8) channel sets, and the unrotated four-channel set
      (15, mode 6), mom_whole + mom_unpack equal the sums over the 16 texels of the channels as the fit sees them
      (slot c < 3 = colour c, or alpha where the rotation put it; slot 3 = alpha or colour rot - 1; slots outside the
      channel set zero; an opaque block's alpha plane is the constant 255), and lo / hi of the rotated alpha equal the
      table entry of channel (rot + 3) & 3;
  partition fits: for the 16-bit texel masks of a subset (random ones, single texels, all but one), the packed moments
      of the subset taken from the table's by mom_sub equal the sums over the other texels, field by field, with the
      block's own channel set (alpha terms zero when opaque) -- and every packed field stays inside its bits.
Blocks: seeded random ones (opaque and with alpha) plus a flat block, a block with one flat half, a constant alpha that
is not 255, channels that reach 0 and 255, all zero and all 255."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuttlefish_amd", "csrc")

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "bc7_packed.h"

static uint64_t st = 20240607;
static uint32_t rnd() { st = st*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 32); }

/* plain sums over the texels of mask: v[t][c] are the channels as the fit sees them */
static void sums(const uint32_t v[16][4], uint32_t mask, uint32_t s[4], uint32_t q[10])
{
	memset(s, 0, 4*sizeof(uint32_t)); memset(q, 0, 10*sizeof(uint32_t));
	for (int t = 0; t < 16; ++t) {
		if (!((mask >> t) & 1u)) continue;
		int k = 0;
		for (int c = 0; c < 4; ++c) {
			s[c] += v[t][c];
			for (int d = c; d < 4; ++d) q[k++] += v[t][c]*v[t][d];   /* q00 q01 q02 q03 q11 q12 q13 q22 q23 q33 */
		}
	}
}

/* the table of the kernel's prologue: the block's own channel set applied (alpha zero when opaque) */
static void table(const uint32_t px[16][4], bool opaque, uint32_t T[CF_MOM_WORDS])
{
	uint32_t v[16][4], s[4], q[10];
	for (int t = 0; t < 16; ++t) for (int c = 0; c < 4; ++c) v[t][c] = (opaque && c == 3) ? 0u : px[t][c];
	sums(v, 0xFFFFu, s, q);
	T[0] = q[0] | (s[0] << 20); T[1] = q[4] | (s[1] << 20); T[2] = q[7] | (s[2] << 20); T[3] = q[9] | (s[3] << 20);
	T[4] = q[1]; T[5] = q[2]; T[6] = q[3]; T[7] = q[5]; T[8] = q[6]; T[9] = q[8];
}

static int same(const char* what, int blk, uint32_t rot, uint32_t chm, const uint32_t s[4], const uint32_t q[10], const uint32_t rs[4], const uint32_t rq[10])
{
	if (!memcmp(s, rs, 16) && !memcmp(q, rq, 40)) return 1;
	printf("%s differs: block %d rot %u chm %u\n", what, blk, rot, chm);
	for (int i = 0; i < 4; ++i) printf(" s%d %u/%u", i, s[i], rs[i]);
	for (int i = 0; i < 10; ++i) printf(" q%d %u/%u", i, q[i], rq[i]);
	printf("\n");
	return 0;
}

int main()
{
	unsigned long whole = 0, parts = 0, opaque_n = 0, flat_subsets = 0;
	for (int blk = 0; blk < 4000; ++blk) {
		uint32_t px[16][4];
		const int kind = blk < 8 ? blk : 8 + (int)(rnd() % 4);
		const uint32_t base[4] = {rnd() & 255u, rnd() & 255u, rnd() & 255u, rnd() & 255u};
		for (int t = 0; t < 16; ++t) for (int c = 0; c < 4; ++c) {
			uint32_t x;
			switch (kind) {
				case 0: x = base[c]; break;                                        /* flat, with alpha */
				case 1: x = c == 3 ? 255u : base[c]; break;                        /* flat, opaque */
				case 2: x = t < 8 ? base[c] : (rnd() & 255u); if (c == 3) x = 255u; break;   /* one flat half */
				case 3: x = c == 3 ? 77u : (rnd() & 255u); break;                  /* constant alpha, not 255 */
				case 4: x = t == 3 ? 0u : (t == 12 ? 255u : (rnd() & 255u)); break;  /* every channel reaches 0 and 255 */
				case 5: x = 0u; break;
				case 6: x = 255u; break;
				case 7: x = c == 3 ? (t == 5 ? 254u : 255u) : 255u; break;         /* largest sums, alpha just not opaque */
				case 8: x = rnd() & 255u; break;                                   /* noise with alpha */
				case 9: x = c == 3 ? 255u : (rnd() & 255u); break;                 /* opaque noise */
				case 10: x = c == 3 ? 255u : ((base[c] + (rnd() % 9)) & 255u); break;   /* smooth, opaque */
				default: x = (base[c] + (uint32_t)t*(1u + (uint32_t)c)) & 255u; break;    /* ramps with alpha */
			}
			px[t][c] = x;
		}
		bool opaque = true;
		for (int t = 0; t < 16; ++t) opaque = opaque && px[t][3] == 255u;
		opaque_n += opaque;
		uint32_t T[CF_MOM_WORDS];
		table(px, opaque, T);
		/* per-channel extremes as the prologue builds them: byte_lohi of each planar row word, then over the rows */
		uint32_t lohi[4];
		for (int c = 0; c < 4; ++c) {
			uint32_t lo = 255u, hi = 0u;
			for (int r = 0; r < 4; ++r) {
				const uint32_t w = px[4*r][c] | (px[4*r + 1][c] << 8) | (px[4*r + 2][c] << 16) | (px[4*r + 3][c] << 24);
				const uint32_t lh = byte_lohi(w);
				lo = (lh & 255u) < lo ? (lh & 255u) : lo;
				hi = (lh >> 8) > hi ? (lh >> 8) : hi;
			}
			lohi[c] = lo | (hi << 8);
		}
		/* whole-block fits */
		for (uint32_t rot = 0; rot < 4u; ++rot) {
			for (int cs = 0; cs < 3; ++cs) {
				const uint32_t chm = cs == 0 ? 7u : (cs == 1 ? 8u : 15u);
				if (chm == 15u && rot != 0u) continue;
				uint32_t v[16][4];
				uint32_t alo = 255u, ahi = 0u;
				for (int t = 0; t < 16; ++t) {
					for (uint32_t c = 0; c < 3u; ++c) v[t][c] = (rot != 0u && c == rot - 1u) ? px[t][3] : px[t][c];
					v[t][3] = rot == 0u ? px[t][3] : px[t][rot - 1u];
					alo = v[t][3] < alo ? v[t][3] : alo;
					ahi = v[t][3] > ahi ? v[t][3] : ahi;
					for (uint32_t c = 0; c < 4u; ++c) if (!((chm >> c) & 1u)) v[t][c] = 0u;
				}
				uint32_t rs[4], rq[10], W[CF_MOM_WORDS], s[4], q[10];
				sums(v, 0xFFFFu, rs, rq);
				mom_whole(T, opaque, rot, chm, W);
				mom_unpack(W, s, q);
				if (!same("mom_whole", blk, rot, chm, s, q, rs, rq)) return 1;
				if (lohi[(rot + 3u) & 3u] != (alo | (ahi << 8))) { printf("lo/hi differs: block %d rot %u\n", blk, rot); return 1; }
				++whole;
			}
		}
		/* partition fits: subset 1 summed, subset 0 by packed subtraction; channel set of the block (rot 0) */
		uint32_t v[16][4];
		for (int t = 0; t < 16; ++t) for (int c = 0; c < 4; ++c) v[t][c] = (opaque && c == 3) ? 0u : px[t][c];
		for (int k = 0; k < 40; ++k) {
			uint32_t m1 = k < 16 ? 1u << k : (k < 32 ? 0xFFFFu ^ (1u << (k - 16)) : rnd() & 0xFFFFu);
			if (m1 == 0u || m1 == 0xFFFFu) m1 = 0x00F0u;
			uint32_t s1[4], q1[10], s0[4], q0[10], A[CF_MOM_WORDS], D[CF_MOM_WORDS], s[4], q[10];
			sums(v, m1, s1, q1);
			sums(v, ~m1 & 0xFFFFu, s0, q0);
			A[0] = q1[0] | (s1[0] << 20); A[1] = q1[4] | (s1[1] << 20); A[2] = q1[7] | (s1[2] << 20); A[3] = q1[9] | (s1[3] << 20);
			A[4] = q1[1]; A[5] = q1[2]; A[6] = q1[3]; A[7] = q1[5]; A[8] = q1[6]; A[9] = q1[8];
			for (int i = 0; i < 10; ++i) if (q1[i] >= (1u << 20) || q0[i] >= (1u << 20)) { printf("a product leaves 20 bits\n"); return 1; }
			for (int i = 0; i < 4; ++i) if (s1[i] >= (1u << 12) || s0[i] >= (1u << 12)) { printf("a sum leaves 12 bits\n"); return 1; }
			mom_unpack(A, s, q);
			if (!same("packing", blk, 0, m1, s, q, s1, q1)) return 1;
			mom_sub(T, A, D);
			mom_unpack(D, s, q);
			if (!same("mom_sub", blk, 0, m1, s, q, s0, q0)) return 1;
			/* a flat subset: n q_cc - s_c^2 == 0 in every channel */
			uint32_t n0 = (uint32_t)__builtin_popcount(~m1 & 0xFFFFu);
			flat_subsets += n0*q[0] == s[0]*s[0] && n0*q[4] == s[1]*s[1] && n0*q[7] == s[2]*s[2] && n0*q[9] == s[3]*s[3];
			++parts;
		}
	}
	printf("whole-block fits %lu, partition subsets %lu, opaque blocks %lu, flat subsets %lu\n", whole, parts, opaque_n, flat_subsets);
	return 0;
}
"""


def test_handed_in_moments_equal_per_texel_sums(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "moments.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "moments"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    whole, parts, opaque, flat = (int(v) for v in re.findall(r"\d+", run.stdout)[:4])
    # 9 whole-block fits and 40 subsets per block; both kinds of block and flat subsets occurred
    assert whole == 4000*9 and parts == 4000*40, run.stdout
    assert 1000 < opaque < 3000 and flat > 40, run.stdout
