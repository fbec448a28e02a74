"""Two exact trims of the unit-weight BC7 fit (csrc/bc7_packed.h) and the pack table (csrc/bc7_pack.h), on the CPU.
DESIGN.md section 4.1, twelfth step.

A stand-alone program (its own main, host compiler) includes bc7_packed.h and checks, against plain twins:

search_key_sum_error -- an assignment's error from the SUM of its texels' masked keys, the weights' sum taken off and
one shift, instead of a shift and an add per texel.  Whole assignments of 16 texels are walked the way assign_lsq_lane
does (raw texel ^ 0x80 against the un-rotated palette ^ 0x80, C = 0, eight entries per lane, mode 6's two halves met by
the smaller key, keys of texels outside the subset zeroed, 32-bit wrapping arithmetic) and the error is formed three
ways: per texel (pp_sum' + sum of key >> 8), from the key sum (the weights' sum by four dot products over the row
words of key_row_weights), and by a plain search (smallest error, then smallest weight) in 64 bits.  All three must
agree; 64-bit shadows hold the ranges the header states (the key sum inside a signed word, key sum - weight sum a multiple
of 256, weight sum <= 1024).  Cases, per index width 2, 3, 4 (4: mode 6, both halves): 2^20 seeded assignments with
random subset masks (empty and full ones included, one in sixteen with equal endpoints); every rotation with channel
sets 7, 8 and 15 (4096 each); bytes 0 / 255, 127 / 128, 0..3 and 252..255 (4096 each).

proj_or_nan / proj_extremes2 -- the extremes of a subset's projections with one select per texel (the value or a quiet
NaN) and two texels per three-operand minimum / maximum, against the scan that selects after every fminf / fmaxf.
(tmin, tmax) must be the same values; only the sign of a zero may differ.  Then the fit's start endpoints, formed as
fit_lane forms them -- d = (tmax - tmin) frac, tmin + d, tmax - d, fmaf(axis, t, mean), clamp255 -- must be BIT-equal for
both scans, with frac 0, 1/16, 1/8 and -1/16: a subset's mean is never -0, so fmaf(axis, +-0, mean) is the same float for
both zeros, and wherever d is not a zero the zero's sign is gone after tmin + d.  Cases: 2^18 seeded subsets of random
texels and axes (components of both signs, zeros of both signs among them); all-equal subsets (every projection the same
value, and exactly +-0 when the texels equal the mean); subsets of two texels; exact ties (pairs of equal texels); axes
with zero components so that +0 and -0 projections meet; empty subsets keep the start values."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuttlefish_amd", "csrc")

PROGRAM = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "bc7_packed.h"
static uint64_t st = 424242123456789ull;
static uint32_t rnd() { st = st*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 32); }
static uint32_t dot4(uint32_t a, uint32_t b)
{
	uint32_t s = 0;
	for (int c = 0; c < 4; ++c) s += ((a >> (8*c)) & 255u)*((b >> (8*c)) & 255u);
	return s;
}
static int fail(const char* what, long long a, long long b) { printf("%s: %lld %lld\n", what, a, b); return 1; }
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

/* ---- the error from the key sum ---- */
static unsigned long nassign = 0, nempty = 0, nfull = 0, nflat = 0, nm6 = 0, nneg = 0;
static long long ksum_min = 0, ksum_max = 0;

static int assignment(const uint32_t (&raw)[16], uint32_t e0, uint32_t e1, uint32_t rot, uint32_t chm, uint32_t ib, uint32_t mask)
{
	const int halves = ib == 4u ? 2 : 1, have = 1 << ib;
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
		const int B = mfma_entry_base((int)((dot4(craw, craw) << 8) | w), dot4(craw, 0x01010101u), 9);
		base[k] = valid ? B : CF_BC7_NO_ENTRY;
		pxor[k] = craw ^ 0x80808080u;
	}
	uint32_t pp_sum = 0, bias = 0;
	for (int t = 0; t < 16; ++t) {
		if (!((mask >> t) & 1u)) continue;
		const uint32_t p = slots(raw[t], rot, chm);
		pp_sum += dot4(p, p);
		bias += dot4(raw[t], 0x01010101u);
	}
	const uint32_t pp_new = search_pp_fold(pp_sum, bias);
	uint32_t err_texel = pp_new, ksum = 0, wrow[4];
	long long err_plain = 0, ksum64 = 0, wsum64 = 0;
	const int m512 = -512;
	for (int r = 0; r < 4; ++r) {
		uint32_t kn[4];
		for (int j = 0; j < 4; ++j) {
			const int t = 4*r + j;
			const bool in = (mask >> t) & 1u;
			const uint32_t ax = raw[t] ^ 0x80808080u;
			int bn = 0x7FFFFFFF;
			for (int h = 0; h < halves; ++h) {
				int hb = 0x7FFFFFFF;
				for (int k = 8*h; k < 8*h + 8; ++k) {
					int M = 0;
					for (int c = 0; c < 4; ++c) M += sb8(ax, c)*sb8(pxor[k], c);
					const int v = key_min_form(M, m512, base[k]);
					if (v < hb) hb = v;
				}
				/* each lane of the pair takes the other's key when it is smaller: both end with the same */
				if (hb < bn) bn = hb;
			}
			const uint32_t p = slots(raw[t], rot, chm);
			long long be = 0; int bw = 0, bk = -1;
			for (int k = 0; k < have; ++k) {
				const long long e = (long long)dot4(pslot[k], pslot[k]) - 2ll*dot4(p, pslot[k]);
				if (bk < 0 || e < be || (e == be && (int)pw[k] < bw)) { be = e; bw = (int)pw[k]; bk = k; }
			}
			if ((bn & 255) != bw) return fail("weight byte", bn & 255, bw);
			kn[j] = in ? (uint32_t)bn : 0u;
			err_texel += (uint32_t)((int)kn[j] >> 8);
			ksum += kn[j];
			ksum64 += (long long)(int)kn[j];
			if (in) {
				err_plain += (long long)dot4(p, p) + be;
				wsum64 += bw;
				if ((int)kn[j] < 0) ++nneg;
			}
		}
		wrow[r] = key_row_weights(kn[0], kn[1], kn[2], kn[3]);
	}
	uint32_t wsum = 0;
	for (int r = 0; r < 4; ++r) wsum += dot4(wrow[r], 0x01010101u);
	if ((long long)wsum != wsum64 || wsum > 1024u) return fail("the weights' sum", wsum, wsum64);
	if (ksum64 != (long long)(int)ksum) return fail("the key sum leaves a signed word", ksum64, (int)ksum);
	if (ksum64 <= -(1ll << 30) || ksum64 >= (1ll << 31)) return fail("range of the key sum", ksum64, 0);
	if (((ksum64 - wsum64) & 255) != 0) return fail("key sum - weight sum is no multiple of 256", ksum64, wsum64);
	if (ksum64 < ksum_min) ksum_min = ksum64;
	if (ksum64 > ksum_max) ksum_max = ksum64;
	const uint32_t err_sum = search_key_sum_error(pp_new, ksum, wsum);
	if (err_plain < 0 || err_plain >= (1ll << 22)) return fail("range of the plain error", err_plain, 0);
	if (err_sum != err_texel || (long long)err_sum != err_plain) {
		printf("errors differ: per texel %u key sum %u plain %lld (ksum %lld wsum %u)\n", err_texel, err_sum, err_plain, ksum64, wsum);
		return 1;
	}
	++nassign; nempty += mask == 0; nfull += mask == 0xFFFFu; nm6 += halves == 2;
	return 0;
}

/* kind: 0 random bytes, 1 bytes 0 / 255, 2 bytes 127 / 128, 3 bytes 0..3, 4 bytes 252..255 */
static uint32_t word_of(int kind)
{
	const uint32_t r = rnd();
	uint32_t v = 0;
	for (int c = 0; c < 4; ++c) {
		const uint32_t b = (r >> (8*c)) & 255u;
		const uint32_t x = kind == 0 ? b : (kind == 1 ? ((b & 1u) ? 255u : 0u) : (kind == 2 ? 127u + (b & 1u) : (kind == 3 ? (b & 3u) : 252u + (b & 3u))));
		v |= x << (8*c);
	}
	return v;
}
static int one(int kind, uint32_t ib, int it, int rotsel, int chmsel)
{
	uint32_t raw[16];
	const bool opq = (it & 4) != 0 && kind != 3;
	for (int t = 0; t < 16; ++t) {
		raw[t] = word_of(kind);
		if (opq) raw[t] |= 0xFF000000u;
	}
	uint32_t e0 = word_of(kind), e1 = word_of(kind);
	if ((it & 15) == 8) { e1 = e0; ++nflat; }
	uint32_t rot = 0, chm, mask;
	if (rotsel >= 0) {
		/* the planes of modes 4 / 5 and mode 6: the whole block */
		rot = (uint32_t)rotsel;
		chm = ib == 4u ? 15u : (chmsel == 0 ? 7u : (chmsel == 1 ? 8u : 15u));
		mask = 0xFFFFu;
	} else {
		bool opaque = true;
		for (int t = 0; t < 16; ++t) opaque = opaque && (raw[t] >> 24) == 255u;
		chm = opaque ? 7u : 15u;
		mask = rnd() & 0xFFFFu;
		if ((it & 255) == 1) mask = 0;
		if ((it & 255) == 2) mask = 0xFFFFu;
	}
	return assignment(raw, e0, e1, rot, chm, ib, mask);
}

/* ---- the projection extremes ---- */
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float clamp255(float x) { return x < 0.0f ? 0.0f : (x > 255.0f ? 255.0f : x); }
static unsigned long nproj = 0, nallequal = 0, ntwo = 0, ntie = 0, nzero_both = 0, nsign = 0, nprojempty = 0, nzero_extreme = 0;

static int extremes(const uint32_t (&px)[16], const float (&axis)[4], uint32_t mask)
{
	uint32_t n = 0, s[4] = {0, 0, 0, 0};
	for (int t = 0; t < 16; ++t)
		if ((mask >> t) & 1u) { ++n; for (int c = 0; c < 4; ++c) s[c] += (px[t] >> (8*c)) & 255u; }
	float mean[4];
	for (int c = 0; c < 4; ++c) mean[c] = n ? (float)s[c]*(1.0f/(float)n) : 0.0f;
	float amin = 3.0e38f, amax = -3.0e38f, bmin = 3.0e38f, bmax = -3.0e38f;
	bool pz = false, nz = false, alleq = true;
	float first = 0.0f; bool have = false;
	for (int r = 0; r < 4; ++r) {
		float tm[4];
		for (int j = 0; j < 4; ++j) {
			const uint32_t p = px[4*r + j];
			const bool m = (mask >> (4*r + j)) & 1u;
			float t = axis[0]*((float)(p & 255u) - mean[0]);
			t = fmaf(axis[1], (float)((p >> 8) & 255u) - mean[1], t);
			t = fmaf(axis[2], (float)((p >> 16) & 255u) - mean[2], t);
			t = fmaf(axis[3], (float)(p >> 24) - mean[3], t);
			/* the scan the kernel had: a select after every minimum */
			amin = m ? fminf(amin, t) : amin;
			amax = m ? fmaxf(amax, t) : amax;
			tm[j] = proj_or_nan(t, m);
			if (m) {
				if (bits(t) == 0u) pz = true;
				if (bits(t) == 0x80000000u) nz = true;
				if (!have) { first = t; have = true; } else if (t != first) alleq = false;
			}
		}
		proj_extremes2(bmin, bmax, tm[0], tm[1]);
		proj_extremes2(bmin, bmax, tm[2], tm[3]);
	}
	if (!(amin == bmin) || !(amax == bmax)) return fail("extremes differ", bits(amin) ^ bits(bmin), bits(amax) ^ bits(bmax));
	if (bits(amin) != bits(bmin) || bits(amax) != bits(bmax)) {
		if (amin != 0.0f && bits(amin) != bits(bmin)) return fail("tmin differs beyond the sign of zero", bits(amin), bits(bmin));
		if (amax != 0.0f && bits(amax) != bits(bmax)) return fail("tmax differs beyond the sign of zero", bits(amax), bits(bmax));
		++nsign;
	}
	if (n == 0) {
		if (bmin != 3.0e38f || bmax != -3.0e38f) return fail("an empty subset moved the start values", bits(bmin), bits(bmax));
		++nprojempty;
	}
	if (n && alleq && (bmin != first || bmax != first)) return fail("all-equal subset", bits(bmin), bits(first));
	/* the start endpoints, as fit_lane forms them */
	const float fracs[4] = {0.0f, 0.0625f, 0.125f, -0.0625f};
	for (int f = 0; f < 4 && n; ++f) {
		const float da = (amax - amin)*fracs[f], db = (bmax - bmin)*fracs[f];
		const float a0 = amin + da, a1 = amax - da, b0 = bmin + db, b1 = bmax - db;
		for (int c = 0; c < 4; ++c) {
			const float xa0 = fmaf(axis[c], a0, mean[c]), xb0 = fmaf(axis[c], b0, mean[c]);
			const float xa1 = fmaf(axis[c], a1, mean[c]), xb1 = fmaf(axis[c], b1, mean[c]);
			if (bits(xa0) != bits(xb0) || bits(xa1) != bits(xb1)) return fail("endpoint before the clamp", bits(xa0) ^ bits(xb0), bits(xa1) ^ bits(xb1));
			if (bits(clamp255(xa0)) != bits(clamp255(xb0)) || bits(clamp255(xa1)) != bits(clamp255(xb1)))
				return fail("endpoint after clamp255", bits(clamp255(xa0)), bits(clamp255(xb0)));
		}
	}
	++nproj; nallequal += n > 1 && alleq; ntwo += n == 2; nzero_both += pz && nz;
	nzero_extreme += n && (bmin == 0.0f || bmax == 0.0f);
	return 0;
}
static float axis_component(int kind)
{
	const uint32_t r = rnd();
	if (kind == 1) {                        /* zeros of both signs and +-1 */
		const float v[4] = {0.0f, -0.0f, 1.0f, -1.0f};
		return v[r & 3u];
	}
	const float m = (float)(r >> 8)*(1.0f/16777216.0f);
	return (r & 1u) ? -m : m;
}
static int one_proj(int it)
{
	uint32_t px[16];
	float axis[4];
	const int shape = it & 7;      /* 0..2 random, 3 all equal, 4 two texels, 5 ties, 6 zero axis components, 7 flat with them */
	for (int t = 0; t < 16; ++t) px[t] = rnd();
	uint32_t mask = rnd() & 0xFFFFu;
	if ((it & 1023) == 9) mask = 0;
	for (int c = 0; c < 4; ++c) axis[c] = axis_component(shape >= 6 ? 1 : 0);
	if (shape == 3 || shape == 7)
		for (int t = 1; t < 16; ++t) px[t] = px[0];
	if (shape == 4) {
		const uint32_t a = rnd() & 15u, b = (a + 1u + rnd() % 15u) & 15u;
		mask = (1u << a) | (1u << b);
	}
	if (shape == 5) {
		for (int t = 0; t < 16; t += 2) px[t + 1] = px[t];
		ntie += 1;
	}
	if (shape == 6) {
		/* one channel varies, symmetric about its mean, the others are constant: projections +-x and, with the
		   channel's axis component zero, products of both signs of zero */
		const uint32_t c = rnd() & 3u, base = rnd();
		for (int t = 0; t < 16; ++t) {
			const uint32_t v = 100u + 20u*(uint32_t)(t & 3);
			px[t] = (base & ~(255u << (8u*c))) | (v << (8u*c));
		}
		mask = 0xFFFFu;
	}
	return extremes(px, axis, mask);
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
	}
	for (int it = 0; it < (1 << 18); ++it)
		if (one_proj(it)) return 1;
	printf("assignments %lu empty %lu full %lu flat %lu mode6 %lu negkeys %lu ksum_min %lld ksum_max %lld\n",
		nassign, nempty, nfull, nflat, nm6, nneg, -ksum_min, ksum_max);
	printf("projections %lu allequal %lu two %lu ties %lu zero_both %lu sign_differs %lu proj_empty %lu zero_extreme %lu\n",
		nproj, nallequal, ntwo, ntie, nzero_both, nsign, nprojempty, nzero_extreme);
	return 0;
}
"""


PACK_PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "bc7_pack.h"
static uint64_t st = 99887766554433ull;
static uint32_t rnd() { st = st*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 32); }
static constexpr cf_bc7_pack_table T = cf_bc7_make_pack();      /* the generator runs in the host compiler */
static_assert(T.w[0] == cf_bc7_cand_word(0), "row 0 is mode 6");
struct Field { uint32_t val, off; bool have; };

/* the layout as pack_block_group wrote it out, branch by branch: slot f of candidate id, for a texel t with `before`
   anchors in front of it, endpoint orders swmask / sws, the candidate's column wcol and the texel's two indices */
static Field plain(uint32_t id, uint32_t f, uint32_t t, uint32_t before, uint32_t swmask, uint32_t sws,
	const uint32_t (&wcol)[8], uint32_t idxv, uint32_t idxs)
{
	uint32_t mode, part = 0, rot = 0, isel = 0;
	if (id == 0u) mode = 6;
	else if (id < 5u) { mode = 5; rot = id - 1u; }
	else if (id < 13u) { mode = 4; rot = (id - 5u) & 3u; isel = (id - 5u) >> 2; }
	else if (id < 128u) { mode = 1; part = id - 64u; }
	else if (id < 192u) { mode = 3; part = id - 128u; }
	else if (id < 256u) { mode = 0; part = id - 192u; }
	else if (id < 320u) { mode = 2; part = id - 256u; }
	else { mode = 7; part = id - 320u; }
	const uint32_t ns  = (0x21112323u >> (4u*mode)) & 15u;
	const uint32_t pbn = (0x60006664u >> (4u*mode)) & 15u;
	const uint32_t cb  = (0x57757564u >> (4u*mode)) & 15u;
	const uint32_t ab  = (0x57860000u >> (4u*mode)) & 15u;
	const uint32_t pk  = (0x11001021u >> (4u*mode)) & 15u;
	const uint32_t ib  = (0x24222233u >> (4u*mode)) & 15u;
	const uint32_t ib2 = (0x00230000u >> (4u*mode)) & 15u;
	uint32_t iba = ib2;
	const bool swapsets = mode == 4u && isel != 0u;
	if (swapsets) iba = 2u;
	const uint32_t ne = 2u*ns;
	const uint32_t hdr = mode + 1u + pbn + ((mode == 4u || mode == 5u) ? 2u : 0u) + (mode == 4u ? 1u : 0u);
	const uint32_t base_pb = hdr + ne*(3u*cb + ab);
	const uint32_t npb = pk == 1u ? ne : (pk == 2u ? 2u : 0u);
	const uint32_t baseA = base_pb + npb;
	const uint32_t baseB = baseA + 16u*ib - ns;
	uint32_t val = 0, off = 0;
	bool have = false;
	if (f < 16u) {
		val = swapsets ? idxs : idxv;
		off = baseA + t*ib - before;
		have = true;
	} else if (f < 32u) {
		val = swapsets ? idxv : idxs;
		off = baseB + t*ib2 - (t > 0u ? 1u : 0u);
		have = ib2 != 0u;
	} else if (f < 56u) {
		const uint32_t g = f - 32u;
		const uint32_t ch = g/ne, e = g - ch*ne;
		const uint32_t es = e ^ ((swmask >> (e >> 1)) & 1u);
		const uint32_t qw = wcol[es];
		if (ch < 3u) {
			val = (qw >> (8u*ch)) & 255u;
			off = hdr + (ch*ne + e)*cb;
			have = true;
		} else if (ch == 3u && ab) {
			const uint32_t sq = wcol[4u + ((e ^ sws) & 1u)];
			val = (iba ? sq : qw) >> 24;
			off = hdr + 3u*ne*cb + e*ab;
			have = true;
		}
	} else if (f < 62u) {
		const uint32_t e = f - 56u;
		const uint32_t pbw = wcol[6];
		if (pk == 1u && e < ne) {
			val = (pbw >> (e ^ ((swmask >> (e >> 1)) & 1u))) & 1u;
			off = base_pb + e;
			have = true;
		} else if (pk == 2u && e < 2u) {
			val = (pbw >> (2u*e)) & 1u;
			off = base_pb + e;
			have = true;
		}
	} else if (f == 62u) {
		val = (1u << mode) | (part << (mode + 1u)) | (rot << (mode + 1u + pbn)) | (isel << (mode + 1u + pbn + 2u));
		if (!(mode == 4u || mode == 5u))
			val = (1u << mode) | (part << (mode + 1u));
		off = 0;
		have = true;
	}
	Field r = {have ? val : 0u, have ? off : 0u, have};
	return r;
}

/* the same slot from the table, as the kernel reads it */
static Field tabled(uint32_t id, uint32_t f, uint32_t before, uint32_t swmask, uint32_t sws,
	const uint32_t (&wcol)[8], uint32_t idxv, uint32_t idxs)
{
	const uint32_t* row = T.w + cf_bc7_cand_index(id)*CF_PACK_ROW;
	const uint32_t cw = row[0];
	const uint32_t mode = CF_CAND_MODE(cw), ns = CF_CAND_NS(cw);
	const uint32_t part = ns > 1u ? id & 63u : 0u;
	const uint32_t pbn = cf_bc7_pack_pbn(mode);
	uint32_t hval = (1u << mode) | (part << (mode + 1u));
	if (CF_CAND_P45(cw))
		hval = (1u << mode) | (CF_CAND_ROT(cw) << (mode + 1u + pbn)) | (CF_CAND_ISEL(cw) << (mode + 1u + pbn + 2u));
	const uint32_t swall = swmask | (sws << 3);
	const uint32_t s = row[1u + f];
	const uint32_t kind = CF_PACK_KIND(s);
	const uint32_t sbit = (swall >> CF_PACK_ORDER(s)) & 1u;
	const uint32_t wi = CF_PACK_WORD(s) ^ (CF_PACK_FLIPW(s) & sbit);
	if (wi > 6u) { Field bad = {0xFFFFFFFFu, 0xFFFFFFFFu, false}; return bad; }
	const uint32_t cval = (wcol[wi] >> (CF_PACK_SHIFT(s) ^ (CF_PACK_FLIPS(s) & sbit))) & (CF_PACK_BYTE(s) ? 255u : 1u);
	uint32_t val = kind == CF_PACK_KIND_COL ? cval : (kind == CF_PACK_KIND_HDR ? hval : (kind == CF_PACK_KIND_IDX1 ? idxv : idxs));
	val = CF_PACK_HAVE(s) ? val : 0u;
	Field r = {val, CF_PACK_HAVE(s) ? CF_PACK_OFF(s) - (f < 16u ? before : 0u) : 0u, CF_PACK_HAVE(s) != 0u};
	return r;
}

int main()
{
	unsigned long nslots = 0, nids = 0, nhave = 0, nmodes = 0, nrot = 0, nisel = 0;
	uint32_t seen_modes = 0;
	for (uint32_t id = 0; id < 384u; ++id) {
		if (id >= 13u && id < 64u) continue;          /* no candidate has these ids */
		const uint32_t cw = T.w[cf_bc7_cand_index(id)*CF_PACK_ROW];
		if (cw != cf_bc7_cand_word(id)) { printf("head word of id %u\n", id); return 1; }
		seen_modes |= 1u << CF_CAND_MODE(cw);
		nrot += CF_CAND_ROT(cw) != 0u; nisel += CF_CAND_ISEL(cw) != 0u;
		const uint32_t iba = CF_CAND_IB2(cw);
		for (uint32_t swmask = 0; swmask < 8u; ++swmask)
			for (uint32_t sws = 0; sws < 2u; ++sws) {
				if (sws && !iba) continue;             /* the kernel's sws is 0 without a scalar plane */
				uint32_t wcol[8];
				for (int k = 0; k < 8; ++k) wcol[k] = rnd();
				for (uint32_t f = 0; f < 64u; ++f) {
					const uint32_t t = f & 15u, before = f < 16u ? rnd() % (t < 3u ? t + 1u : 4u) : 0u;
					const uint32_t idxv = rnd() & 15u, idxs = rnd() & 7u;
					const Field a = plain(id, f, t, before, swmask, sws, wcol, idxv, idxs);
					const Field b = tabled(id, f, before, swmask, sws, wcol, idxv, idxs);
					if (a.have != b.have || a.val != b.val || a.off != b.off) {
						printf("id %u slot %u swmask %u sws %u: plain (%u, %u, %d) table (%u, %u, %d)\n", id, f, swmask, sws,
							a.val, a.off, (int)a.have, b.val, b.off, (int)b.have);
						return 1;
					}
					if (a.have && f >= 16u && a.off > 127u) { printf("offset of id %u slot %u\n", id, f); return 1; }
					++nslots; nhave += a.have;
				}
			}
		++nids;
	}
	for (uint32_t m = 0; m < 8u; ++m) nmodes += (seen_modes >> m) & 1u;
	printf("ids %lu slots %lu have %lu modes %lu rotated %lu selector %lu\n", nids, nslots, nhave, nmodes, nrot, nisel);
	return 0;
}
"""


def test_pack_table_equals_the_written_out_field_layout(tmp_path):
    """csrc/bc7_pack.h: every slot of every candidate id (every mode, partition, rotation and index selector), under
    every endpoint order, gives the value, the bit offset and the presence that pack_block_group's branches gave."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "pack_table.cpp"
    src.write_text(PACK_PROGRAM)
    exe = tmp_path / "pack_table"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    v = {k: int(x) for k, x in re.findall(r"([a-z_0-9]+) (\d+)", run.stdout)}
    assert v["ids"] == 13 + 5*64 and v["modes"] == 8, run.stdout
    assert v["rotated"] == 3 + 6 and v["selector"] == 4, run.stdout
    # 8 subset orders for every id, doubled where a scalar plane has an order of its own (ids 1..12)
    assert v["slots"] == (8*(1 + 5*64) + 16*12)*64 and v["have"] > v["slots"]//3, run.stdout


def test_key_sum_error_and_nan_masked_extremes_equal_their_plain_twins(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "shelved_trims.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "shelved_trims"
    # (no contraction: fmaf is spelled where the kernel fuses, as in the device build)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), str(src), "-lm"])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    v = {k: int(x) for k, x in re.findall(r"([a-z_0-9]+) (\d+)", run.stdout)}
    per_width = (1 << 20) + 12*4096 + 4*4096
    assert v["assignments"] == 3*per_width, run.stdout
    assert v["empty"] >= 3*3000 and v["full"] >= 3*12*4096 and v["flat"] >= 3*(1 << 16) and v["mode6"] == per_width, run.stdout
    # the sum stays inside the stated range (no key of the search without its C operand lies below zero)
    assert v["negkeys"] == 0 and v["ksum_min"] == 0 and 0 < v["ksum_max"] < (1 << 31), run.stdout
    assert v["projections"] == 1 << 18, run.stdout
    assert v["allequal"] >= 1 << 14 and v["two"] >= 1 << 14 and v["ties"] == 1 << 15, run.stdout
    assert v["zero_both"] >= 1 and v["zero_extreme"] >= 1 << 12 and v["proj_empty"] >= 200, run.stdout
