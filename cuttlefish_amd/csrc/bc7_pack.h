// The field slots of a packed BC7 block as a table per (candidate shape, slot), with the shape's candidate word at its
// head (bc7_encode.hip: pack_block_group).  A slot's bit offset, whether the mode has it and where its value comes from
// depend on the mode and, for the two index fields of mode 4, on the index selector -- not on the partition or the
// rotation -- so the ladder of compares on the slot number and the offset arithmetic that followed it are one table word
// per slot, in one row per shape (bc7_cand.h: cf_bc7_cand_index, 18 shapes).  What stays per block:
// the anchors' fix-up of the first index field's offsets, the endpoint swaps and the header's value.
// Plain constexpr C++: a host program includes this file and compares every slot with the layout written out
// field by field (tests/test_bc7_shelved_trims.py).
#ifndef CFHIP_BC7_PACK_H
#define CFHIP_BC7_PACK_H

#include <stdint.h>
#include "bc7_cand.h"

// Slots f of a block (pack_block_group): 0..15 first index field of texel f, 16..31 second index field of texel f - 16,
// 32..55 endpoint fields (channel-major), 56..61 p-bits, 62 the header (mode bit, partition, rotation, selector); 63 none.
// Slot word:
//   bits  0..7   bit offset of the field in the block (first index field: before the anchors' fix-up, which takes up to three
//                bits off, so the last texel's may stand at 128 or 129 here)
//   bit   8      the mode has this slot
//   bits  9..10  kind: 0 an index of the vector plane (of the only plane), 1 an index of the scalar plane, 2 a field of the
//                candidate's column, 3 the header
//   bits 11..13  kind 2: column word that holds the value (0..3 endpoints e of the subsets, 4..5 the scalar plane's, 6 p-bits)
//   bits 14..18  kind 2: the value's shift in that word
//   bit  19      kind 2: the value is a byte (otherwise one bit)
//   bits 20..21  kind 2: whose endpoint order applies: subset 0..2, or 3 the scalar plane
//   bit  22      kind 2: a swapped order flips bit 0 of the column word's number (endpoint fields)
//   bit  23      kind 2: a swapped order flips bit 0 of the shift (p-bits per endpoint)
#define CF_PACK_OFF(s) ((s) & 255u)
#define CF_PACK_HAVE(s) (((s) >> 8) & 1u)
#define CF_PACK_KIND(s) (((s) >> 9) & 3u)
#define CF_PACK_WORD(s) (((s) >> 11) & 7u)
#define CF_PACK_SHIFT(s) (((s) >> 14) & 31u)
#define CF_PACK_BYTE(s) (((s) >> 19) & 1u)
#define CF_PACK_ORDER(s) (((s) >> 20) & 3u)
#define CF_PACK_FLIPW(s) (((s) >> 22) & 1u)
#define CF_PACK_FLIPS(s) (((s) >> 23) & 1u)
#define CF_PACK_KIND_IDX1 0u
#define CF_PACK_KIND_IDX2 1u
#define CF_PACK_KIND_COL 2u
#define CF_PACK_KIND_HDR 3u

// Per mode: partition bits, widths of the two index fields as packed, alpha bits as packed
constexpr uint32_t cf_bc7_pack_pbn(uint32_t mode) { return (0x60006664u >> (4u*mode)) & 15u; }     // partition bits
constexpr uint32_t cf_bc7_pack_ib1(uint32_t mode) { return (0x24222233u >> (4u*mode)) & 15u; }
constexpr uint32_t cf_bc7_pack_ib2(uint32_t mode) { return (0x00230000u >> (4u*mode)) & 15u; }
constexpr uint32_t cf_bc7_pack_ab(uint32_t mode) { return (0x57860000u >> (4u*mode)) & 15u; }      // alpha bits as packed
// a candidate id of shape row i (cf_bc7_cand_index): the id itself below 13, partition 0 of the mode otherwise
constexpr uint32_t cf_bc7_pack_id_of(uint32_t i) { return i < 13u ? i : (i - 12u)*64u; }

constexpr uint32_t cf_bc7_pack_slot(uint32_t shape, uint32_t f)
{
	const uint32_t w = cf_bc7_cand_word(cf_bc7_pack_id_of(shape));
	const uint32_t mode = CF_CAND_MODE(w);
	const bool swapsets = mode == 4u && CF_CAND_ISEL(w) != 0u;   // the first index field then holds the scalar plane's indices
	const uint32_t ns = CF_CAND_NS(w), cb = CF_CAND_CB(w), pk = CF_CAND_PBK(w);
	const bool p45 = CF_CAND_P45(w) != 0u;
	const uint32_t ab = cf_bc7_pack_ab(mode), ib = cf_bc7_pack_ib1(mode), ib2 = cf_bc7_pack_ib2(mode);
	const uint32_t ne = 2u*ns;
	const uint32_t hdr = mode + 1u + cf_bc7_pack_pbn(mode) + (p45 ? 2u : 0u) + (mode == 4u ? 1u : 0u);
	const uint32_t base_pb = hdr + ne*(3u*cb + ab);
	const uint32_t npb = pk == 1u ? ne : (pk == 2u ? 2u : 0u);
	const uint32_t baseA = base_pb + npb, baseB = baseA + 16u*ib - ns;
	uint32_t off = 0, have = 0, kind = 0, word = 0, shift = 0, byte = 0, order = 0, flipw = 0, flips = 0;
	if (f < 16u) {
		off = baseA + f*ib; have = 1; kind = swapsets ? CF_PACK_KIND_IDX2 : CF_PACK_KIND_IDX1;
	} else if (f < 32u) {
		const uint32_t t = f - 16u;
		off = baseB + t*ib2 - (t > 0u ? 1u : 0u); have = ib2 != 0u ? 1u : 0u; kind = swapsets ? CF_PACK_KIND_IDX1 : CF_PACK_KIND_IDX2;
	} else if (f < 56u) {
		const uint32_t g = f - 32u, ch = g/ne, e = g - ch*ne;
		kind = CF_PACK_KIND_COL; byte = 1;
		if (ch < 3u) {
			off = hdr + (ch*ne + e)*cb; have = 1; word = e; shift = 8u*ch; order = e >> 1; flipw = 1;
		} else if (ch == 3u && ab) {
			// modes 4 / 5: the scalar plane's endpoints are parked in column words 4, 5 (byte 3), in its own order
			off = hdr + 3u*ne*cb + e*ab; have = 1; shift = 24; flipw = 1;
			word = p45 ? 4u + e : e; order = p45 ? 3u : e >> 1;
		}
	} else if (f < 62u) {
		const uint32_t e = f - 56u;
		kind = CF_PACK_KIND_COL; word = 6;
		if (pk == 1u && e < ne) { off = base_pb + e; have = 1; shift = e; order = e >> 1; flips = 1; }
		else if (pk == 2u && e < 2u) { off = base_pb + e; have = 1; shift = 2u*e; }
	} else if (f == 62u) {
		have = 1; kind = CF_PACK_KIND_HDR;
	}
	if (!have)
		off = kind = word = shift = byte = order = flipw = flips = 0;
	return off | (have << 8) | (kind << 9) | (word << 11) | (shift << 14) | (byte << 19) | (order << 20) | (flipw << 22) | (flips << 23);
}

// Row of a shape: word 0 its candidate word, words 1..64 the slots 0..63.
#define CF_PACK_ROW 65u
struct cf_bc7_pack_table { uint32_t w[CF_CAND_TABLE_N*CF_PACK_ROW]; };
constexpr cf_bc7_pack_table cf_bc7_make_pack()
{
	cf_bc7_pack_table t = {};
	for (uint32_t i = 0; i < CF_CAND_TABLE_N; ++i) {
		t.w[i*CF_PACK_ROW] = cf_bc7_cand_word(cf_bc7_pack_id_of(i));
		for (uint32_t f = 0; f < 64u; ++f)
			t.w[i*CF_PACK_ROW + 1u + f] = cf_bc7_pack_slot(i, f);
	}
	return t;
}

#endif
