"""The unit-weight BC7 selector search without the C operand of its matrix-pipe instruction (csrc/bc7_packed.h:
search_pp_fold, search_bias_part, lohi_pack / lohi_rawsum), on the CPU.  DESIGN.md section 4.1, eleventh step.

A stand-alone program (its own main, host compiler) includes bc7_packed.h and walks whole assignments of 16 texels the way
assign_lsq_lane does -- raw texel ^ 0x80 against the un-rotated palette ^ 0x80, eight entries per lane, mode 6's two halves
met by the smaller key, keys of texels outside the subset zeroed, the error summed from key >> 8 on top of the fit's
constant, everything in 32-bit wrapping arithmetic -- in three forms:
  today   C = 128 sum_c a_c per texel, constant pp_sum = sum over the subset of sum_c p_c^2
  new     C = 0, constant pp_sum' = search_pp_fold(pp_sum, bias)
  plain   per texel the entry of smallest error cc - 2 dt, then smallest weight; error = sum over the subset of |p - c|^2
and asserts the same entry per texel, the same weight word per row (key_row_weights) and the same assignment error.
64-bit shadows check the ranges bc7_packed.h states: |sum a'b'| <= 2^16; key' in (-2^26, 2^27) and equal to its 64-bit
value; CF_BC7_NO_ENTRY - 512 sum a'b' in (2^29, 2^31); both operands of the 24-bit multiply-add fit 24 bits; key' - key =
65536 A_t with A_t the sum of the texel's four raw bytes.
The bias comes from where the kernel takes it, by the fit's role: a whole-block fit (any rotation, channel set 7, 8 or 15)
from the table word, the byte sum of the block's 16 planar words packed above a channel's extremes as the kernel's
prologue stores it (lohi_pack; both fields must come back); a partition fit (rotation 0, channel set 7 on an opaque
block, 15 otherwise) from search_bias_part over its own subset sums.  Both are compared with the direct sum of the
subset's raw bytes.
Cases, per index width 2, 3, 4 (4: mode 6, both halves): 2^20 seeded assignments, one in four a whole-block fit, the rest
partition fits with random subset masks (empty and full ones included), one in sixteen with equal endpoints (every entry
ties); every rotation with channel sets 7, 8 and 15 (4096 each); blocks of bytes 0 / 255, of bytes 127 / 128, dark blocks
of bytes 0..3 (pp_sum' must have wrapped below zero in at least one) and blocks of bytes 252..255 (the largest bias),
4096 each, and 16 blocks each of all bytes 255 and all bytes 0, whole-block and partition fits alternating."""
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
static uint64_t st = 977123456789ull;
static uint32_t rnd() { st = st*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 32); }
static uint32_t dot4(uint32_t a, uint32_t b)
{
	uint32_t s = 0;
	for (int c = 0; c < 4; ++c) s += ((a >> (8*c)) & 255u)*((b >> (8*c)) & 255u);
	return s;
}
static int fail(const char* what, long long a, long long b) { printf("%s: %lld %lld\n", what, a, b); return 1; }
/* a word as a fit of rotation rot and channel set chm sees it: colour rot - 1 and alpha change places, slots not coded are zero */
static uint32_t slots(uint32_t v, uint32_t rot, uint32_t chm)
{
	uint32_t b[4] = {v & 255u, (v >> 8) & 255u, (v >> 16) & 255u, v >> 24};
	if (rot) { const uint32_t t = b[rot - 1u]; b[rot - 1u] = b[3]; b[3] = t; }
	uint32_t r = 0;
	for (int c = 0; c < 4; ++c) r |= ((chm >> c) & 1u ? b[c] : 0u) << (8*c);
	return r;
}
static uint32_t unrot(uint32_t v, uint32_t rot)
{
	uint32_t b[4] = {v & 255u, (v >> 8) & 255u, (v >> 16) & 255u, v >> 24};
	if (rot) { const uint32_t t = b[rot - 1u]; b[rot - 1u] = b[3]; b[3] = t; }
	return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
}
static int sb8(uint32_t w, int c) { return (int)(int8_t)(w >> (8*c)); }

static unsigned long nassign = 0, nwhole = 0, npart = 0, nwrapped = 0, nempty = 0, nfull = 0, nflat = 0, nopaque = 0, nm6 = 0;
static unsigned long nwrapped_dark = 0, maxbias = 0;

/* One assignment.  raw: the block's 16 raw texels; e0 / e1: raw endpoint words; whole: the fit's role. */
static int assignment(const uint32_t (&raw)[16], uint32_t e0, uint32_t e1, uint32_t rot, uint32_t chm, uint32_t ib,
	uint32_t mask, bool whole, bool dark)
{
	bool opaque = true;
	for (int t = 0; t < 16; ++t) opaque = opaque && (raw[t] >> 24) == 255u;
	const int halves = ib == 4u ? 2 : 1, have = 1 << ib;
	/* the palette once per assignment: slot order for the plain search, raw channel order ^ 0x80 for the matrix pipe */
	const uint32_t s0 = slots(e0, rot, chm), s1 = slots(e1, rot, chm);
	const PalLine line = pal_line(unrot(s0, rot), unrot(s1, rot));
	uint32_t pslot[16], pw[16], pxor[16];
	int base[16];
	for (int k = 0; k < 8*halves; ++k) {
		const bool valid = k < have;
		const uint32_t w = valid ? cf_bc7_weight(ib, (uint32_t)k) : 0u;
		pslot[k] = pal_word(s0, s1, w);
		pw[k] = w;
		const uint32_t craw = pal_at(line, w);
		if (craw != unrot(pslot[k], rot)) return fail("un-rotated palette", craw, pslot[k]);
		const int B = mfma_entry_base((int)((dot4(craw, craw) << 8) | w), dot4(craw, 0x01010101u), 9);
		base[k] = valid ? B : CF_BC7_NO_ENTRY;
		pxor[k] = craw ^ 0x80808080u;
	}
	/* the constant of the fit and the bias, from where the kernel takes them */
	uint32_t pp_sum = 0, s[4] = {0, 0, 0, 0}, n = 0;
	unsigned long long direct = 0;
	for (int t = 0; t < 16; ++t) {
		if (!((mask >> t) & 1u)) continue;
		const uint32_t p = slots(raw[t], rot, chm);
		pp_sum += dot4(p, p);
		for (int c = 0; c < 4; ++c) s[c] += (p >> (8*c)) & 255u;
		direct += dot4(raw[t], 0x01010101u);
		++n;
	}
	uint32_t bias;
	if (whole) {
		/* the table word as the kernel's prologue forms it: the 16 planar words (channel c of the four texels of row r)
		   summed byte by byte, packed above the extremes of a channel (the rotated alpha's, here) */
		uint32_t rs = 0, lo = 255u, hi = 0u;
		const uint32_t ach = rot ? rot - 1u : 3u;
		for (int r = 0; r < 4; ++r)
			for (uint32_t c = 0; c < 4; ++c) {
				uint32_t pw = 0;
				for (int j = 0; j < 4; ++j) pw |= ((raw[4*r + j] >> (8u*c)) & 255u) << (8*j);
				rs += dot4(pw, 0x01010101u);
				if (c == ach) {
					const uint32_t lh = byte_lohi(pw);
					lo = (lh & 255u) < lo ? (lh & 255u) : lo; hi = (lh >> 8) > hi ? (lh >> 8) : hi;
				}
			}
		const uint32_t word = lohi_pack(lo | (hi << 8), rs);
		if ((word & 255u) != lo || lohi_hi(word) != hi) return fail("the extremes beside the raw sum", word, lo | (hi << 8));
		bias = lohi_rawsum(word);
		++nwhole;
	} else {
		/* (as the kernel decides it: the fit does not code alpha, which only an opaque block's partition fit does not) */
		if (opaque != !(chm & 8u)) return fail("a partition fit's channel set", chm, opaque);
		bias = search_bias_part(s[0], s[1], s[2], s[3], n, !(chm & 8u));
		++npart;
	}
	if ((unsigned long long)bias != direct) return fail(whole ? "table word" : "partition bias", bias, (long long)direct);
	if (bias > maxbias) maxbias = bias;
	const uint32_t pp_new = search_pp_fold(pp_sum, bias);
	if ((long long)pp_sum - 256ll*(long long)bias < 0) {
		if ((int)pp_new >= 0) return fail("pp_sum' did not wrap", pp_new, bias);
		++nwrapped; nwrapped_dark += dark;
	}
	uint32_t err_old = pp_sum, err_new = pp_new;
	long long err_plain = 0;
	const int m512 = -512;
	for (int r = 0; r < 4; ++r) {
		uint32_t ko[4], kn[4], wplain = 0;
		for (int j = 0; j < 4; ++j) {
			const int t = 4*r + j;
			const bool in = (mask >> t) & 1u;
			const uint32_t ax = raw[t] ^ 0x80808080u;
			const long long A = dot4(raw[t], 0x01010101u);
			int ro[2], rn[2], io[2], in_[2];
			for (int h = 0; h < halves; ++h) {
				int bo = 0x7FFFFFFF, bn = 0x7FFFFFFF, xo = -1, xn = -1;
				for (int k = 8*h; k < 8*h + 8; ++k) {
					long long M = 0;
					for (int c = 0; c < 4; ++c) M += sb8(ax, c)*sb8(pxor[k], c);
					if (M > (1ll << 16) || M < -(1ll << 16)) return fail("range of sum a'b'", M, k);
					if (M >= (1ll << 23) || M < -(1ll << 23)) return fail("24-bit operand", M, k);
					const long long D = M + 128*A;
					const int vo = key_min_form((int)D, m512, base[k]);
					const int vn = key_min_form((int)M, m512, base[k]);
					const long long x = (long long)base[k] - 512ll*M;
					if (x != (long long)vn) return fail("key' leaves 32 bits", x, vn);
					if (k < have) {
						if (x >= (1ll << 27) || x <= -(1ll << 26)) return fail("range of key'", x, k);
						if (x - (long long)vo != 65536ll*A) return fail("key' - key", x - vo, 65536ll*A);
					} else if (x <= (1ll << 29) || x >= (1ll << 31))
						return fail("a missing entry's key'", x, k);
					if (vo < bo) { bo = vo; xo = k; }
					if (vn < bn) { bn = vn; xn = k; }
				}
				ro[h] = bo; rn[h] = bn; io[h] = xo; in_[h] = xn;
			}
			int bo = ro[0], bn = rn[0], xo = io[0], xn = in_[0];
			if (halves == 2) {
				/* each lane of the pair takes the other's key when it is smaller: both end with the same */
				if (ro[1] < bo) { bo = ro[1]; xo = io[1]; }
				if (rn[1] < bn) { bn = rn[1]; xn = in_[1]; }
			}
			/* the plain search: smallest error, then smallest weight */
			const uint32_t p = slots(raw[t], rot, chm);
			long long be = 0; int bw = 0, bk = -1;
			for (int k = 0; k < have; ++k) {
				const long long e = (long long)dot4(pslot[k], pslot[k]) - 2ll*dot4(p, pslot[k]);
				if (bk < 0 || e < be || (e == be && (int)pw[k] < bw)) { be = e; bw = (int)pw[k]; bk = k; }
			}
			if (xo != xn || xn != bk) return fail("winning entry", xn, bk);
			if ((bo & 255) != (bn & 255) || (bn & 255) != bw) return fail("weight byte", bn & 255, bw);
			if ((long long)(bn >> 8) != (long long)(bo >> 8) + 256ll*A) return fail("key' >> 8", bn >> 8, bo >> 8);
			ko[j] = in ? (uint32_t)bo : 0u;
			kn[j] = in ? (uint32_t)bn : 0u;
			err_old += (uint32_t)((int)ko[j] >> 8);
			err_new += (uint32_t)((int)kn[j] >> 8);
			if (in) {
				err_plain += (long long)dot4(p, p) + be;
				wplain |= (uint32_t)bw << (8*j);
			}
		}
		const uint32_t wo = key_row_weights(ko[0], ko[1], ko[2], ko[3]), wn = key_row_weights(kn[0], kn[1], kn[2], kn[3]);
		if (wo != wn || wn != wplain) return fail("weight word of a row", wn, wplain);
	}
	if (err_plain < 0 || err_plain >= (1ll << 22)) return fail("range of the plain error", err_plain, 0);
	if (err_old != err_new || (long long)err_new != err_plain) {
		printf("errors differ: today %u new %u plain %lld (pp_sum %u, pp_sum' %u, bias %u)\n", err_old, err_new, err_plain, pp_sum, pp_new, bias);
		return 1;
	}
	++nassign; nempty += mask == 0; nfull += mask == 0xFFFFu; nopaque += opaque; nm6 += halves == 2;
	return 0;
}

/* kind: 0 random bytes, 1 bytes 0 / 255, 2 bytes 127 / 128, 3 bytes 0..3, 4 bytes 252..255, 5 all bytes 255, 6 all bytes 0 */
static uint32_t word_of(int kind)
{
	const uint32_t r = rnd();
	uint32_t v = 0;
	for (int c = 0; c < 4; ++c) {
		const uint32_t b = (r >> (8*c)) & 255u;
		const uint32_t x = kind == 5 ? 255u : kind == 6 ? 0u : kind == 0 ? b : (kind == 1 ? ((b & 1u) ? 255u : 0u) : (kind == 2 ? 127u + (b & 1u) : (kind == 3 ? (b & 3u) : 252u + (b & 3u))));
		v |= x << (8*c);
	}
	return v;
}
/* one seeded case of a kind; it: running number (role, flat endpoints, the forced masks) */
static int one(int kind, uint32_t ib, int it, int rotsel, int chmsel)
{
	uint32_t raw[16];
	const bool whole = rotsel >= 0 || (it & 3) == 0;
	const bool opq = (it & 4) != 0 && kind != 3;
	for (int t = 0; t < 16; ++t) {
		raw[t] = word_of(kind);
		if (opq) raw[t] |= 0xFF000000u;
	}
	uint32_t e0 = word_of(kind), e1 = word_of(kind);
	if ((it & 15) == 8) { e1 = e0; ++nflat; }
	uint32_t rot, chm, mask;
	if (whole) {
		/* mode 6 and the planes of modes 4 / 5: the whole block by role */
		const uint32_t ci = rotsel >= 0 ? (uint32_t)chmsel : rnd() % 3u;
		rot = rotsel >= 0 ? (uint32_t)rotsel : rnd() & 3u;
		chm = ib == 4u ? 15u : (ci == 0 ? 7u : (ci == 1 ? 8u : 15u));
		if (ib == 4u && rotsel < 0) rot = 0;
		mask = 0xFFFFu;
	} else {
		rot = 0;
		bool opaque = true;   /* (by the block's content, as the kernel's ballot: a drawn block may be opaque by chance) */
		for (int t = 0; t < 16; ++t) opaque = opaque && (raw[t] >> 24) == 255u;
		chm = opaque ? 7u : 15u;
		mask = rnd() & 0xFFFFu;
		if ((it & 255) == 1) mask = 0;
		if ((it & 255) == 2) mask = 0xFFFFu;
	}
	return assignment(raw, e0, e1, rot, chm, ib, mask, whole, kind == 3);
}
int main()
{
	for (uint32_t ib = 2; ib <= 4; ++ib) {
		for (int it = 0; it < (1 << 20); ++it)
			if (one(0, ib, it, -1, 0)) return 1;
		for (int rot = 0; rot < 4; ++rot)
			for (int ci = 0; ci < 3; ++ci)
				for (int it = 0; it < 4096; ++it)
					if (one(0, ib, it, rot, ci)) return 1;
		for (int kind = 1; kind <= 4; ++kind)
			for (int it = 0; it < 4096; ++it)
				if (one(kind, ib, 2*it + (it >> 11), -1, 0)) return 1;
		for (int kind = 5; kind <= 6; ++kind)
			for (int it = 0; it < 16; ++it)
				if (one(kind, ib, it, -1, 0)) return 1;
	}
	printf("assignments %lu whole %lu partition %lu wrapped %lu wrapped_dark %lu empty %lu full %lu flat %lu opaque %lu mode6 %lu maxbias %lu\n",
		nassign, nwhole, npart, nwrapped, nwrapped_dark, nempty, nfull, nflat, nopaque, nm6, maxbias);
	return 0;
}
"""


def test_search_without_c_operand_equals_todays_and_the_plain_search(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "search_bias.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "search_bias"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    v = {k: int(x) for k, x in re.findall(r"([a-z_0-9]+) (\d+)", run.stdout)}
    per_width = (1 << 20) + 12*4096 + 4*4096 + 2*16
    assert v["assignments"] == 3*per_width, run.stdout
    assert v["whole"] + v["partition"] == v["assignments"] and v["whole"] > 3*(1 << 18) and v["partition"] > 3*(1 << 19), run.stdout
    # a dark block's pp_sum' lies below zero before the keys bring the sum back into range
    assert v["wrapped_dark"] >= 1 and v["wrapped"] >= v["wrapped_dark"], run.stdout
    assert v["empty"] >= 3*3000 and v["full"] > v["whole"] and v["flat"] >= 3*(1 << 16), run.stdout
    assert v["opaque"] > 3*(1 << 18) and v["mode6"] == per_width, run.stdout
    # the largest bias: a block of bytes 255, 64 * 255
    assert v["maxbias"] == 64*255, run.stdout
