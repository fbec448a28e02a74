"""The whole-word identities of csrc/bc7_packed.h against the per-byte formulas of the BC7 format, on the CPU.

A small stand-alone program includes the header (its functions are plain inline functions for a host compiler) and
compares, with the per-byte formulas restated in the program:
  dequant1      every (t, v), t = 4..8, v < 2^t;
  dequant_rgb   every colour triple for t = 4, 5 and 6, 2^20 seeded triples for t = 7 and 8 -- and, with each of them,
                dequant_word under every alpha width (not coded, 4..8) with a seeded alpha code, and with the colours
                not coded;
  code_word     both shifts, both p-bits, on seeded field words (fields of at most 7 bits under a shift);
  pal_word      every weight of the 2-, 3- and 4-bit index tables on 2^20 seeded endpoint pairs and on the 256 pairs of
                words whose bytes are each 0 or 255.
The program prints the number of comparisons of each group and fails on the first difference."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuttlefish_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdint.h>
#include "bc7_packed.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
	rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)(rng_state >> 32);
}

/* the format's formulas, one byte at a time */
static uint32_t ref_dequant(uint32_t v, uint32_t t) { return ((v << (8u - t)) | (v >> (2u*t - 8u))) & 255u; }
static uint32_t ref_pal(uint32_t a, uint32_t b, uint32_t w) { return ((64u - w)*a + w*b + 32u) >> 6; }

static int fail(const char* what, uint32_t a, uint32_t b, uint32_t c, uint32_t got, uint32_t want)
{
	printf("MISMATCH %s(%08x, %08x, %u): %08x, per byte %08x\n", what, a, b, c, got, want);
	return 1;
}

static unsigned long n_rgb = 0, n_word = 0;
static int check_triple(uint32_t word, uint32_t t)
{
	uint32_t want = 0;
	for (int c = 0; c < 3; ++c)
		want |= ref_dequant((word >> (8*c)) & 255u, t) << (8*c);
	const uint32_t got = dequant_rgb(word, t);
	++n_rgb;
	if (got != want)
		return fail("dequant_rgb", word, 0, t, got, want);
	/* the whole word under every alpha width; ta = 0: alpha not coded (its byte still holds a p-bit) */
	for (uint32_t ta = 0; ta <= 8; ta = ta ? ta + 1 : 4) {
		const uint32_t a = ta ? rnd() & ((1u << ta) - 1u) : rnd() & 1u;
		const uint32_t w4 = (word & 0x00FFFFFFu) | (a << 24);
		const uint32_t wa = ta ? ref_dequant(a, ta) << 24 : 0u;
		++n_word;
		if (dequant_word(w4, t, ta) != (want | wa))
			return fail("dequant_word", w4, t, ta, dequant_word(w4, t, ta), want | wa);
		/* colours not coded: their bytes hold at most a p-bit */
		const uint32_t w1 = (w4 & 0xFF010101u);
		if (dequant_word(w1, 0, ta) != wa)
			return fail("dequant_word, alpha alone", w1, 0, ta, dequant_word(w1, 0, ta), wa);
	}
	return 0;
}

int main(void)
{
	unsigned long n = 0;
	for (uint32_t t = 4; t <= 8; ++t)
		for (uint32_t v = 0; v < (1u << t); ++v, ++n)
			if (dequant1(v, t) != ref_dequant(v, t))
				return fail("dequant1", v, 0, t, dequant1(v, t), ref_dequant(v, t));
	printf("dequant1 %lu\n", n);

	for (uint32_t t = 4; t <= 6; ++t)
		for (uint32_t i = 0; i < (1u << (3*t)); ++i) {
			const uint32_t m = (1u << t) - 1u;
			if (check_triple((i & m) | (((i >> t) & m) << 8) | (((i >> (2*t)) & m) << 16), t))
				return 1;
		}
	for (uint32_t t = 7; t <= 8; ++t)
		for (uint32_t i = 0; i < (1u << 20); ++i) {
			const uint32_t m = ((1u << t) - 1u)*0x010101u;
			if (check_triple(rnd() & m, t))
				return 1;
		}
	printf("dequant_rgb %lu\ndequant_word %lu\n", n_rgb, n_word);

	n = 0;
	for (uint32_t S = 0; S < 2; ++S)
		for (uint32_t P = 0; P < 2; ++P)
			for (uint32_t i = 0; i < (1u << 16); ++i, ++n) {
				const uint32_t q = rnd() & (S ? 0x7F7F7F7Fu : 0xFFFFFFFFu);
				uint32_t want = 0;
				for (int c = 0; c < 4; ++c)
					want |= ((((q >> (8*c)) & 255u) << S) | P) << (8*c);
				if (code_word(q, S, P) != want)
					return fail("code_word", q, S, P, code_word(q, S, P), want);
			}
	printf("code_word %lu\n", n);

	static const uint32_t weights[28] = {0, 21, 43, 64, 0, 9, 18, 27, 37, 46, 55, 64,
		0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64};
	n = 0;
	for (uint32_t i = 0; i < (1u << 20) + 256u; ++i) {
		uint32_t e0, e1;
		if (i < 256u) {      /* the corners: every byte of both words 0 or 255 */
			e0 = e1 = 0;
			for (int c = 0; c < 4; ++c) {
				e0 |= ((i >> c) & 1u ? 255u : 0u) << (8*c);
				e1 |= ((i >> (4 + c)) & 1u ? 255u : 0u) << (8*c);
			}
		} else {
			e0 = rnd();
			e1 = rnd();
		}
		for (int k = 0; k < 28; ++k, ++n) {
			uint32_t want = 0;
			for (int c = 0; c < 4; ++c)
				want |= ref_pal((e0 >> (8*c)) & 255u, (e1 >> (8*c)) & 255u, weights[k]) << (8*c);
			if (pal_word(e0, e1, weights[k]) != want)
				return fail("pal_word", e0, e1, weights[k], pal_word(e0, e1, weights[k]), want);
		}
	}
	printf("pal_word %lu\n", n);
	return 0;
}
"""


def test_packed_helpers_equal_the_per_byte_formulas(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "identities.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "identities"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    counts = dict((line.split()[0], int(line.split()[1])) for line in run.stdout.splitlines())
    assert counts["dequant1"] == 16 + 32 + 64 + 128 + 256
    assert counts["dequant_rgb"] == (1 << 12) + (1 << 15) + (1 << 18) + 2 * (1 << 20)
    assert counts["dequant_word"] == 6 * counts["dequant_rgb"]      # alpha not coded and 4..8 bits, with every triple
    assert counts["code_word"] == 4 << 16
    assert counts["pal_word"] == 28 * ((1 << 20) + 256)
