"""Host side of the thirteenth step of DESIGN.md section 4.1 (csrc/bc7_packed.h: cov_term, cf_put_weights), compiled with the host compiler from the headers the kernel includes.

  covariance   n q_cd - s_c s_d by one fused multiply-add on floats (cov_term) against the integer subtraction and its
               conversion, bit for bit, in float32: 2^20 seeded subsets of n = 1..16 texels (the sums of real bytes),
               2^20 seeded triples (n, q, s_c s_d) drawn over the whole stated range without regard to what texels
               can give, and the extremes: n = 16 with all texels 255, n = 1, and s_c s_d = n q_cd (flat subsets: +0).
  masks        a fit's weights stored into the four weight words its candidate's fits share by and / or with
               cf_put_weights (the p-bit word keeps its read-modify-write, one fit at a time), in every order that keeps a fit's and before its own or, against the read-modify-write of one fit after
               the other: for every partitioned mode (0, 1, 2, 3, 7) and partition, every fit, every index width the
               mode has, and the whole-block fits of modes 6, 4 and 5.

The GPU side is tests/test_gpu_bc7_gather_trims.py."""
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
#include <math.h>
#include "bc7_cand.h"
#include "bc7_packed.h"

static uint64_t st = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { st = st*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 33); }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* the integer form the kernel had */
static float cov_int(uint32_t n, uint32_t q, uint32_t sc, uint32_t sd) { return (float)(int)(n*q - sc*sd); }

static unsigned long ncov = 0, nzero = 0, nneg = 0;
static int cov_check(uint32_t n, uint32_t q, uint32_t sc, uint32_t sd)
{
	const float a = cov_term((float)n, q, (float)sc, (float)sd), b = cov_int(n, q, sc, sd);
	++ncov; nzero += b == 0.0f; nneg += b < 0.0f;
	if (bits(a) != bits(b)) { printf("covariance n %u q %u sc %u sd %u: fma %08x integer %08x\n", n, q, sc, sd, bits(a), bits(b)); return 1; }
	return 0;
}

/* ---- masks ---- */
static const uint16_t P2[64] = CF_BC7_PART2_INIT;
static const uint32_t P3[64] = CF_BC7_PART3_INIT;
static uint32_t subset_mask(uint32_t ns, uint32_t part, uint32_t kf)
{
	uint32_t m = 0;
	for (uint32_t t = 0; t < 16u; ++t) {
		const uint32_t sb = ns == 1u ? 0u : (ns == 2u ? (P2[part] >> t) & 1u : (P3[part] >> (2u*t)) & 3u);
		if (sb == kf) m |= 1u << t;
	}
	return m;
}
static uint32_t bytemask4(uint32_t m) { return ((m*0x00204081u) & 0x01010101u)*0xFFu; }

struct Fit { uint32_t kf, mask, pb, w[4]; };
/* words: [0] unused, [1..4] the weight words (7..10 of the column) */
static void put_rmw(uint32_t (&wd)[5], const Fit& f, bool)
{
	for (uint32_t rr = 0; rr < 4u; ++rr) {
		const uint32_t mb = bytemask4((f.mask >> (4u*rr)) & 15u);
		wd[1 + rr] = (wd[1 + rr] & ~mb) | f.w[rr];
	}
}
static unsigned long nmask = 0, norders = 0;
static int mask_check(uint32_t mode, uint32_t ns, uint32_t part, uint32_t ib, bool pbits)
{
	Fit f[3];
	for (uint32_t k = 0; k < ns; ++k) {
		f[k].kf = k; f[k].mask = subset_mask(ns, part, k); f[k].pb = pbits ? rnd() & 3u : 0u;
		for (uint32_t rr = 0; rr < 4u; ++rr) {
			uint32_t w = 0;
			for (uint32_t j = 0; j < 4u; ++j)       /* a weight of the width's palette in every texel of the fit */
				if ((f[k].mask >> (4u*rr + j)) & 1u) w |= ((rnd() % ((1u << ib))) * 64u / ((1u << ib) - 1u)) << (8u*j);
			f[k].w[rr] = w;
		}
	}
	/* any subset of the fits wins; the others leave their bits as they are */
	for (uint32_t win = 1; win < (1u << ns); ++win) {
		uint32_t start[5], ref[5];
		for (int i = 0; i < 5; ++i) ref[i] = start[i] = rnd();
		for (uint32_t k = 0; k < ns; ++k) if ((win >> k) & 1u) put_rmw(ref, f[k], pbits);
		/* an LDS instruction applies its lanes in some order; the ands are one instruction, the ors the next.  Also the
		   orders in which a whole fit (and, then or) follows another. */
		for (uint32_t order = 0; order < 6u; ++order) {
			static const uint32_t perm[6][3] = {{0,1,2},{0,2,1},{1,0,2},{1,2,0},{2,0,1},{2,1,0}};
			for (uint32_t form = 0; form < 2u; ++form) {
				uint32_t wd[5];
				for (int i = 0; i < 5; ++i) wd[i] = start[i];
				for (uint32_t phase = 0; phase < 2u; ++phase)
					for (uint32_t i = 0; i < 3u; ++i) {
						const uint32_t k = perm[order][i];
						if (k >= ns || !((win >> k) & 1u)) continue;
						if (form == 0u) {            /* all ands, then all ors */
							for (uint32_t rr = 0; rr < 4u; ++rr) {
								const cf_put_masks wm = cf_put_weights(f[k].mask, rr, f[k].w[rr]);
								if (phase == 0u) wd[1 + rr] &= wm.keep; else wd[1 + rr] |= wm.set;
							}
						} else if (phase == 0u) {    /* fit after fit */
							for (uint32_t rr = 0; rr < 4u; ++rr) {
								const cf_put_masks wm = cf_put_weights(f[k].mask, rr, f[k].w[rr]);
								wd[1 + rr] &= wm.keep; wd[1 + rr] |= wm.set;
							}
						}
					}
				++norders;
				for (int i = 0; i < 5; ++i)
					if (wd[i] != ref[i]) {
						printf("masks mode %u part %u ib %u win %u order %u form %u word %d: %08x, read-modify-write %08x\n",
							mode, part, ib, win, order, form, i, wd[i], ref[i]);
						return 1;
					}
			}
		}
	}
	++nmask;
	return 0;
}

int main()
{
	/* seeded subsets of real texels */
	for (uint32_t it = 0; it < (1u << 20); ++it) {
		const uint32_t n = 1u + rnd() % 16u;
		uint32_t sc = 0, sd = 0, q = 0;
		const uint32_t kind = rnd() & 7u;
		const uint32_t fc = rnd() & 255u, fd = rnd() & 255u;
		for (uint32_t t = 0; t < n; ++t) {
			const uint32_t c = kind == 0u ? fc : rnd() & 255u, d = kind == 0u ? fd : (kind == 1u ? c : rnd() & 255u);
			sc += c; sd += d; q += c*d;
		}
		if (cov_check(n, q, sc, sd)) return 1;
	}
	/* the whole stated range: n <= 16, n q < 2^24, s_c s_d < 2^24 */
	for (uint32_t it = 0; it < (1u << 20); ++it) {
		const uint32_t n = 1u + rnd() % 16u;
		const uint32_t q = rnd() % (16u*255u*255u + 1u);
		const uint32_t sc = rnd() % 4081u, sd = rnd() % 4081u;
		if (cov_check(n, q, sc, sd)) return 1;
	}
	/* extremes */
	if (cov_check(16u, 16u*255u*255u, 4080u, 4080u)) return 1;      /* n = 16, all texels 255: 2^24 - 130816 both ways */
	if (cov_check(16u, 16u*255u*255u, 0u, 0u)) return 1;            /* the largest product alone */
	if (cov_check(16u, 0u, 4080u, 4080u)) return 1;                 /* the largest subtrahend alone */
	for (uint32_t c = 0; c < 256u; ++c)
		for (uint32_t d = 0; d < 256u; ++d) {
			if (cov_check(1u, c*d, c, d)) return 1;                      /* n = 1: always zero */
			for (uint32_t n = 2; n <= 16u; n += 7u)
				if (cov_check(n, n*c*d, n*c, n*d)) return 1;             /* flat subset: s_c s_d = n q_cd */
		}
	if (bits(cov_term(7.0f, 7u*9u, 21.0f, 21.0f)) != 0u) { printf("zero is not +0\n"); return 1; }

	/* masks: (mode, subsets, partitions, index width, p-bits) */
	static const uint32_t modes[8][5] = {
		{0, 3, 16, 3, 1}, {1, 2, 64, 3, 1}, {2, 3, 64, 2, 0}, {3, 2, 64, 2, 1}, {7, 2, 64, 2, 1},
		{6, 1, 1, 4, 1}, {4, 1, 1, 2, 0}, {5, 1, 1, 2, 0}
	};
	for (int m = 0; m < 8; ++m)
		for (uint32_t part = 0; part < modes[m][2]; ++part)
			for (uint32_t rep = 0; rep < 8u; ++rep) {
				if (mask_check(modes[m][0], modes[m][1], part, modes[m][3], modes[m][4] != 0u)) return 1;
				if (modes[m][0] == 4u && mask_check(4u, 1u, 0u, 3u, false)) return 1;      /* mode 4's other index width */
			}
	/* a three-subset shape: the masks of its fits are disjoint and cover the block */
	for (uint32_t part = 0; part < 64u; ++part) {
		if ((subset_mask(3, part, 0) | subset_mask(3, part, 1) | subset_mask(3, part, 2)) != 0xFFFFu) { printf("cover\n"); return 1; }
		if ((subset_mask(2, part, 0) ^ subset_mask(2, part, 1)) != 0xFFFFu) { printf("cover2\n"); return 1; }
	}
	printf("covariances %lu zero %lu negative %lu shapes %lu orders %lu\n", ncov, nzero, nneg, nmask, norders);
	return 0;
}
"""


def test_fma_covariance_and_put_masks_equal_their_plain_twins(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "gather_trims.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "gather_trims"
    # (no contraction: the fused operation is spelled where the kernel fuses, as in the device build)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), str(src), "-lm"])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    v = {k: int(x) for k, x in re.findall(r"([a-z_0-9]+) (\d+)", run.stdout)}
    assert v["covariances"] == 2*(1 << 20) + 3 + 65536*(1 + 3), run.stdout
    # flat subsets and n = 1 give zeros; the ranged triples give differences of both signs
    assert v["zero"] >= 65536*4 + (1 << 17) - 4096 and v["negative"] > (1 << 18), run.stdout
    assert v["shapes"] == 8*(16 + 4*64 + 3) + 8, run.stdout
    assert v["orders"] > v["shapes"]*12, run.stdout
