// The candidate word of the BC7 search (bc7_encode.hip, encode_blocks) and the table of fit masks.
// A candidate's id says everything about its shape -- mode, rotation, index selector, subset count, the precisions
// and index width of its fits -- but taking those from the id is a ladder of compares.  The leader lane that stores a
// candidate into its LDS column stores these facts with it, once, in the 26 spare bits of the column's p-bit word
// (word 6: bits 0..5 are the p-bits, every reader masks them and column_put_fit read-modify-writes them).  The
// phases that come back to a stored candidate -- the starts trip before and after its fit, the perturbation pass --
// take their fields from this word with bit-field extracts.  (Lowest and Low have neither phase and store no word.)
// The word describes fit 0 (subset 0, the vector plane, mode 6); the subsets of a partition share everything but
// their texels, and the scalar plane of modes 4 / 5 follows from the vector plane (cf_bc7_cand_fit_of).
// A fit's texels come from one table indexed by (subset count, partition, fit): cf_bc7_make_masks.
// Plain constexpr C++: a host program includes this file and compares every field with the formulas written out id by
// id (tests/test_bc7_cand_words.py).
#ifndef CFHIP_BC7_CAND_H
#define CFHIP_BC7_CAND_H

#include <stdint.h>

// The partition tables of the format: bit t of a two-subset word = subset of texel t, bits 2t..2t+1 of a three-subset word.
#define CF_BC7_PART2_INIT { \
	0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, \
	0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000, \
	0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310, 0x3100, 0x8cce, \
	0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c, \
	0xaaaa, 0xf0f0, 0x5a5a, 0x33cc, 0x3c3c, 0x55aa, 0x9696, 0xa55a, \
	0x73ce, 0x13c8, 0x324c, 0x3bdc, 0x6996, 0xc33c, 0x9966, 0x0660, \
	0x0272, 0x04e4, 0x4e40, 0x2720, 0xc936, 0x936c, 0x39c6, 0x639c, \
	0x9336, 0x9cc6, 0x817e, 0xe718, 0xccf0, 0x0fcc, 0x7744, 0xee22 }
#define CF_BC7_PART3_INIT { \
	0xaa685050, 0x6a5a5040, 0x5a5a4200, 0x5450a0a8, 0xa5a50000, 0xa0a05050, 0x5555a0a0, 0x5a5a5050, \
	0xaa550000, 0xaa555500, 0xaaaa5500, 0x90909090, 0x94949494, 0xa4a4a4a4, 0xa9a59450, 0x2a0a4250, \
	0xa5945040, 0x0a425054, 0xa5a5a500, 0x55a0a0a0, 0xa8a85454, 0x6a6a4040, 0xa4a45000, 0x1a1a0500, \
	0x0050a4a4, 0xaaa59090, 0x14696914, 0x69691400, 0xa08585a0, 0xaa821414, 0x50a4a450, 0x6a5a0200, \
	0xa9a58000, 0x5090a0a8, 0xa8a09050, 0x24242424, 0x00aa5500, 0x24924924, 0x24499224, 0x50a50a50, \
	0x500aa550, 0xaaaa4444, 0x66660000, 0xa5a0a5a0, 0x50a050a0, 0x69286928, 0x44aaaa44, 0x66666600, \
	0xaa444444, 0x54a854a8, 0x95809580, 0x96969600, 0xa85454a8, 0x80959580, 0xaa141414, 0x96960000, \
	0xaaaa1414, 0xa05050a0, 0xa0a5a5a0, 0x96000000, 0x40804080, 0xa9a8a9a8, 0xaaaaaa44, 0x2a4a5254 }

// Candidate word (column word 6).
//   bits  0..5   p-bits of the candidate's fits, bit 2 s + e (not part of the definition below: 0 there)
//   bits  6..8   mode
//   bits  9..10  rotation (modes 4 / 5)
//   bit  11      index selector (mode 4)
//   bits 12..13  subsets
//   bits 14..15  fits: the subsets, or the two planes of modes 4 / 5
//   bit  16      planes45: the candidate is a vector plane and a scalar plane
//   bits 17..19  cb of fit 0: bits of the colour channels
//   bits 20..23  ab of fit 0: bits of the alpha channel, 0 when fit 0 does not code it
//   bits 24..25  pbk: 0 no p-bits, 1 per endpoint, 2 shared
//   bits 26..28  ib of fit 0: index width
//   bit  29      fit 0 codes the fourth channel (chm 15, otherwise 7)
//   bits 30..31  index width of the scalar plane, 0 when there is none
#define CF_CAND_PB_BITS 6u
#define CF_CAND_PB_MASK 63u
#define CF_CAND_MODE(w) (((w) >> 6) & 7u)
#define CF_CAND_ROT(w) (((w) >> 9) & 3u)
#define CF_CAND_ISEL(w) (((w) >> 11) & 1u)
#define CF_CAND_NS(w) (((w) >> 12) & 3u)
#define CF_CAND_NFITS(w) (((w) >> 14) & 3u)
#define CF_CAND_P45(w) (((w) >> 16) & 1u)
#define CF_CAND_CB(w) (((w) >> 17) & 7u)
#define CF_CAND_AB(w) (((w) >> 20) & 15u)
#define CF_CAND_PBK(w) (((w) >> 24) & 3u)
#define CF_CAND_IB(w) (((w) >> 26) & 7u)
#define CF_CAND_A4(w) (((w) >> 29) & 1u)
#define CF_CAND_IB2(w) ((w) >> 30)

// The word of candidate id (ids: 0 mode 6; 1..4 mode 5 x rotation; 5..12 mode 4 x rotation x index selector;
// 64 + p, 128 + p, 192 + p, 256 + p, 320 + p: modes 1, 3, 0, 2, 7 on partition p).
constexpr uint32_t cf_bc7_cand_word(uint32_t id)
{
	uint32_t mode = 7, rot = 0, isel = 0;
	if (id == 0u) mode = 6;
	else if (id < 5u) { mode = 5; rot = id - 1u; }
	else if (id < 13u) { mode = 4; rot = (id - 5u) & 3u; isel = (id - 5u) >> 2; }
	else if (id < 128u) mode = 1;
	else if (id < 192u) mode = 3;
	else if (id < 256u) mode = 0;
	else if (id < 320u) mode = 2;
	const bool p45 = mode == 4u || mode == 5u;
	const uint32_t ns = (0x21112323u >> (4u*mode)) & 15u, nfits = p45 ? 2u : ns;
	uint32_t cb = (0x57757564u >> (4u*mode)) & 15u, ab = (0x57860000u >> (4u*mode)) & 15u;
	uint32_t ib = (0x24222233u >> (4u*mode)) & 15u, ib2 = 0;
	const uint32_t pbk = (0x11001021u >> (4u*mode)) & 15u;
	if (p45) {
		// fit 0 is the vector plane: no alpha; mode 4's selector swaps the index widths of the planes
		ab = 0;
		ib = (mode == 4u && isel) ? 3u : 2u;
		ib2 = mode == 4u ? (isel ? 2u : 3u) : 2u;
	}
	return (mode << 6) | (rot << 9) | (isel << 11) | (ns << 12) | (nfits << 14) | ((p45 ? 1u : 0u) << 16) |
		(cb << 17) | (ab << 20) | (pbk << 24) | (ib << 26) | ((ab ? 1u : 0u) << 29) | (ib2 << 30);
}

// The words as a table, one entry per shape: ids 0..12, then one per mode of the partition ids (id >> 6 = 1..5).
#define CF_CAND_TABLE_N 18u
constexpr uint32_t cf_bc7_cand_index(uint32_t id) { return id < 13u ? id : 12u + (id >> 6); }
struct cf_bc7_cand_table { uint32_t w[CF_CAND_TABLE_N]; };
constexpr cf_bc7_cand_table cf_bc7_make_cands()
{
	cf_bc7_cand_table t = {};
	for (uint32_t id = 0; id < 13u; ++id)
		t.w[cf_bc7_cand_index(id)] = cf_bc7_cand_word(id);
	for (uint32_t id = 64u; id < 384u; id += 64u)
		t.w[cf_bc7_cand_index(id)] = cf_bc7_cand_word(id);
	return t;
}

// Fit kf of the candidate with word w and id `id`, everything but its texels (mi: their entry in the mask table).
struct cf_bc7_cand_fit {
	uint32_t mode, part, rot, isel, ns, nfits, cb, ab, pbk, ib, chm, mi;
	bool m6, planes45, sca;
};

constexpr cf_bc7_cand_fit cf_bc7_cand_fit_of(uint32_t w, uint32_t id, uint32_t kf)
{
	cf_bc7_cand_fit g = {};
	g.mode = CF_CAND_MODE(w); g.rot = CF_CAND_ROT(w); g.isel = CF_CAND_ISEL(w);
	g.ns = CF_CAND_NS(w); g.nfits = CF_CAND_NFITS(w);
	g.planes45 = CF_CAND_P45(w) != 0u;
	g.m6 = g.mode == 6u;
	// partition ids are 64 m + p; the ids below 64 have one subset and every entry of that row is the whole block
	g.part = g.ns > 1u ? id & 63u : 0u;
	g.sca = g.planes45 && kf == 1u;
	// the scalar plane codes the rotated alpha with one bit more than the vector plane's colours, no p-bits in either
	g.cb = g.sca ? 0u : CF_CAND_CB(w);
	g.ab = g.sca ? CF_CAND_CB(w) + 1u : CF_CAND_AB(w);
	g.pbk = CF_CAND_PBK(w);
	g.ib = g.sca ? CF_CAND_IB2(w) : CF_CAND_IB(w);
	g.chm = g.sca ? 8u : 7u | (CF_CAND_A4(w) << 3);
	g.mi = (g.ns << 8) | ((id & 63u) << 2) | (kf & 3u);
	return g;
}

// Texels of fit kf: [subsets][partition][kf], 16 bits each.  One subset: the whole block in every entry (any id
// below 64 indexes it, and any fit index -- both planes, both palette halves of mode 6).  Row 0 belongs to no candidate:
// it is there so that a word that is none (a column no leader has stored into) indexes the table all the same.
struct cf_bc7_mask_table { uint16_t m[4u*64u*4u]; };
constexpr cf_bc7_mask_table cf_bc7_make_masks()
{
	constexpr uint16_t p2[64] = CF_BC7_PART2_INIT;
	constexpr uint32_t p3[64] = CF_BC7_PART3_INIT;
	cf_bc7_mask_table t = {};
	for (uint32_t p = 0; p < 64u; ++p)
		for (uint32_t kf = 0; kf < 4u; ++kf) {
			uint32_t m3 = 0;
			for (uint32_t x = 0; x < 16u; ++x)
				m3 |= ((p3[p] >> (2u*x)) & 3u) == kf ? 1u << x : 0u;
			t.m[(0u*64u + p)*4u + kf] = 0xFFFFu;
			t.m[(1u*64u + p)*4u + kf] = 0xFFFFu;
			// (a fit index past the subsets belongs to an idle lane; the id ladder before this table gave such a lane subset 1's texels)
			t.m[(2u*64u + p)*4u + kf] = (uint16_t)(kf ? p2[p] : ~p2[p] & 0xFFFFu);
			t.m[(3u*64u + p)*4u + kf] = (uint16_t)m3;
		}
	return t;
}

#endif
