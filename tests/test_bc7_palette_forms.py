"""The palette forms of csrc/bc7_packed.h that the selector search builds once per assignment, on the CPU.

A small stand-alone program includes the header and compares, with the format's formulas restated in the program:
  weight table  every byte of cf_bc7_make_weights() against (k*64 + d/2)/d, d = 2^ib - 1, for ib = 2, 3 and 4 (mode 6:
                entries 0..7 in one row, 8..15 in the other); entries 4..7 of the 2-bit row are 0; weight_row() finds
                the row of every (mode 6, half, index width) and stays inside the table for any width;
  pal_at        pal_at(pal_line(e0, e1), w) against the per-byte (iw*e0 + w*e1 + 32) >> 6 and against pal_word, for
                every weight of the three index tables, on 2^20 seeded endpoint pairs and on the 256 pairs whose bytes
                are each 0 or 255 -- the pairs in which a half of e1 - e0 borrows from the half above it.
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

/* the format's formulas */
static uint32_t ref_weight(uint32_t ib, uint32_t k) { const uint32_t d = (1u << ib) - 1u; return (k*64u + d/2u)/d; }
static uint32_t ref_pal(uint32_t a, uint32_t b, uint32_t w) { return ((64u - w)*a + w*b + 32u) >> 6; }

int main(void)
{
	static const cf_bc7_weight_table T = cf_bc7_make_weights();
	unsigned long n = 0;
	uint32_t weights[28];
	int nw = 0;
	for (uint32_t ib = 2; ib <= 4; ++ib)
		for (uint32_t k = 0; k < (1u << ib); ++k, ++n) {
			const uint32_t row = weight_row(ib == 4u, k >> 3, ib);
			if (row >= CF_BC7_WEIGHT_ROWS) { printf("MISMATCH weight_row(%u, %u): %u\n", ib, k >> 3, row); return 1; }
			const uint32_t got = weight_at(T.w[row][0], T.w[row][1], k & 7u), want = ref_weight(ib, k);
			if (got != want) { printf("MISMATCH weight ib %u k %u: %u, formula %u\n", ib, k, got, want); return 1; }
			weights[nw++] = want;
		}
	/* what a 2-bit fit reads for the entries it does not have, and the rows of widths no fit has */
	if (T.w[0][1] != 0u) { printf("MISMATCH entries 4..7 of the 2-bit row: %08x\n", T.w[0][1]); return 1; }
	for (uint32_t ib = 0; ib < 16u; ++ib)
		for (uint32_t h = 0; h < 4u; ++h)
			if (weight_row(false, h, ib) >= 2u || weight_row(true, h, ib) != 2u + (h & 1u)) {
				printf("MISMATCH weight_row leaves its rows: ib %u half %u\n", ib, h);
				return 1;
			}
	printf("weights %lu\n", n);

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
		const PalLine line = pal_line(e0, e1);
		for (int k = 0; k < 28; ++k, ++n) {
			uint32_t want = 0;
			for (int c = 0; c < 4; ++c)
				want |= ref_pal((e0 >> (8*c)) & 255u, (e1 >> (8*c)) & 255u, weights[k]) << (8*c);
			const uint32_t got = pal_at(line, weights[k]);
			if (got != want || got != pal_word(e0, e1, weights[k])) {
				printf("MISMATCH pal_at(%08x, %08x, %u): %08x, per byte %08x, pal_word %08x\n", e0, e1, weights[k], got, want,
					pal_word(e0, e1, weights[k]));
				return 1;
			}
		}
	}
	printf("pal_at %lu\n", n);
	return 0;
}
"""


def test_palette_forms_equal_the_per_byte_formulas(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "palette_forms.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "palette_forms"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    counts = dict((line.split()[0], int(line.split()[1])) for line in run.stdout.splitlines())
    assert counts["weights"] == 4 + 8 + 16
    assert counts["pal_at"] == 28 * ((1 << 20) + 256)
