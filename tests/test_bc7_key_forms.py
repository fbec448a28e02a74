"""The key of a texel in the BC7 selector search (csrc/bc7_packed.h: key_min_form) against the maximum form the search
had before it, on the CPU.  The maximum form is the reference and is defined here (key_max_form in the program below).

A stand-alone program (its own main, host compiler) includes bc7_packed.h and walks a texel over a palette both ways:
  old   every entry holds -B_k, the texel's value is (dt << 8) - B_k, the largest wins, the key is its negation
  new   every entry holds B_k, the value is B_k - 256 dt, the smallest wins and is the key (what the kernel computes)
with B_k = (cc_k << 7) | w_k, an entry that does not exist at -/+0x3FFFFFFF, the start values -/+0x7FFFFFFF and, for the
sixteen entries of mode 6, the larger / smaller of the two halves' results, as assign_lsq_lane does it.  Compared per
case: the error part U >> 7 (arithmetic shift), the weight U & 127 and the index of the winning entry; both are also
checked against a plain search for the smallest error, the smallest weight among equals.
Cases: 2^20 seeded (texel, palette) pairs per index width 2, 3 and 4 -- one in eight with both endpoints equal in some
or all channels, so that entries tie -- then all 256 palettes whose endpoint bytes are each 0 or 255 against the 16
texels of the same kind, per width, and 2^20 cases of raw (dt, cc) values over the perceptual metric's ranges
(dt < 2^22, cc < 2^22).  Cases in which two entries have the smallest error are counted and must occur."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuttlefish_amd", "csrc")

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "bc7_packed.h"
static uint64_t st = 987654321;
static uint32_t rnd() { st = st*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 32); }
static uint32_t dot4(uint32_t a, uint32_t b)
{
	uint32_t s = 0;
	for (int c = 0; c < 4; ++c) s += ((a >> (8*c)) & 255u)*((b >> (8*c)) & 255u);
	return s;
}
/* the reference: the maximum form, whose entries hold -B */
static int key_max_form(int dt, int negB) { return (dt << 8) + negB; }
static unsigned long ncase = 0, nties = 0;
/* n entries (8: one lane; 16: the two halves of mode 6), of which the first `have` exist */
static int walk(const int* dt, const int* B, int n, int have)
{
	int res_old[2], res_new[2], arg_old[2], arg_new[2];
	const int m256 = -256;
	for (int h = 0; h < n/8; ++h) {
		int bo = -0x7FFFFFFF, bn = 0x7FFFFFFF, ao = -1, an = -1;
		for (int k = 8*h; k < 8*h + 8; ++k) {
			const bool valid = k < have;
			const int vo = key_max_form(dt[k], valid ? -B[k] : -CF_BC7_NO_ENTRY);
			const int vn = key_min_form(dt[k], m256, valid ? B[k] : CF_BC7_NO_ENTRY);
			if (vo > bo) { bo = vo; ao = k; }
			if (vn < bn) { bn = vn; an = k; }
		}
		res_old[h] = bo; res_new[h] = bn; arg_old[h] = ao; arg_new[h] = an;
	}
	int bo = res_old[0], bn = res_new[0], ao = arg_old[0], an = arg_new[0];
	if (n == 16) {
		if (res_old[1] > bo) { bo = res_old[1]; ao = arg_old[1]; }
		if (res_new[1] < bn) { bn = res_new[1]; an = arg_new[1]; }
	}
	const int ko = -bo, kn = bn;
	/* the plain search: smallest error, then smallest weight */
	long long be = 0; int bw = 0, bk = -1, equal = 0;
	for (int k = 0; k < have; ++k) {
		const long long e = (long long)(B[k] >> 7) - 2ll*dt[k];
		const int w = B[k] & 127;
		if (bk < 0 || e < be || (e == be && w < bw)) { be = e; bw = w; bk = k; }
	}
	for (int k = 0; k < have; ++k)
		equal += (long long)(B[k] >> 7) - 2ll*dt[k] == be;
	++ncase; nties += equal > 1;
	if ((ko >> 7) != (kn >> 7) || (ko & 127) != (kn & 127) || ao != an || (long long)(kn >> 7) != be || (kn & 127) != bw || an != bk) {
		printf("differs: old key %d entry %d, new key %d entry %d, plain error %lld weight %d entry %d\n", ko, ao, kn, an, be, bw, bk);
		return 1;
	}
	return 0;
}
static int palette_case(uint32_t e0, uint32_t e1, uint32_t p, uint32_t ib)
{
	int dt[16], B[16];
	const int n = ib == 4u ? 16 : 8, have = 1 << ib;
	for (int k = 0; k < n; ++k) {
		const uint32_t w = k < have ? cf_bc7_weight(ib, (uint32_t)k) : 0u;
		const uint32_t c = pal_word(e0, e1, w);
		dt[k] = (int)dot4(p, c);
		B[k] = (int)((dot4(c, c) << 7) | w);
	}
	return walk(dt, B, n, have);
}
int main()
{
	for (uint32_t ib = 2; ib <= 4; ++ib) {
		for (int it = 0; it < (1 << 20); ++it) {
			uint32_t e0 = rnd(), e1 = rnd();
			const uint32_t p = rnd();
			if ((it & 7) == 0) {          /* equal endpoints in the channels of a random mask: ties */
				const uint32_t m = ((rnd() & 1u) ? 0xFFu : 0u) | ((rnd() & 1u) ? 0xFF00u : 0u) | ((rnd() & 1u) ? 0xFF0000u : 0u) | ((it & 8) ? 0xFF000000u : 0u);
				e1 = (e1 & ~m) | (e0 & m);
				if (it & 16) e1 = e0;
			}
			if (palette_case(e0, e1, p, ib)) return 1;
		}
		for (uint32_t pal = 0; pal < 256; ++pal)
			for (uint32_t t = 0; t < 16; ++t) {
				uint32_t e0 = 0, e1 = 0, p = 0;
				for (int c = 0; c < 4; ++c) {
					e0 |= ((pal >> c) & 1u ? 255u : 0u) << (8*c);
					e1 |= ((pal >> (4 + c)) & 1u ? 255u : 0u) << (8*c);
					p |= ((t >> c) & 1u ? 255u : 0u) << (8*c);
				}
				if (palette_case(e0, e1, p, ib)) return 1;
			}
	}
	const unsigned long unit_cases = ncase, unit_ties = nties;
	for (int it = 0; it < (1 << 20); ++it) {   /* the perceptual metric's ranges, weights of a 3-bit index */
		int dt[8], B[8];
		const uint32_t cc0 = rnd() >> 10, d0 = rnd() >> 10;
		for (int k = 0; k < 8; ++k) {
			const bool near = (it & 3) == 0;    /* entries whose errors differ by little, or not at all */
			const uint32_t cc = near ? cc0 + 2u*(rnd() & 3u) : rnd() >> 10;
			dt[k] = (int)(near ? d0 + (rnd() & 3u) : rnd() >> 10);
			B[k] = (int)((cc << 7) | cf_bc7_weight(3u, (uint32_t)k));
		}
		if (walk(dt, B, 8, 8)) return 1;
	}
	printf("equal on %lu palette cases with %lu ties, %lu raw cases with %lu ties\n", unit_cases, unit_ties, ncase - unit_cases, nties - unit_ties);
	return 0;
}
"""


def test_minimum_form_keys_equal_the_maximum_form(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "keys.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "keys"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    cases, ties, raw, raw_ties = (int(v) for v in re.findall(r"\d+", run.stdout)[:4])
    assert cases == 3*((1 << 20) + 256*16) and raw == 1 << 20, run.stdout
    assert ties > 100000 and raw_ties > 1000, run.stdout
