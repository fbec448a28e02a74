// Lane roles of the BC7 stream trips (bc7_encode.hip, encode_blocks) as two packed words per lane.
// What a lane does in a stream trip depends on the layout (32-lane Lowest, 32-lane Low / Normal, 64-lane High /
// Highest), on the trip st, on whether the lane's half carries alpha and walks the second pass, and on the lane's
// index hl in its half -- on nothing the search computes.  cf_bc7_role_word / cf_bc7_fit_word derive everything from
// those; the kernel reads them from a table built here at compile time (cf_bc7_make_roles), once before the fit and once
// after it.  (Lowest's instance keeps its roles as expressions: its layout folds to constants and the words did not
// pay there.  Its layout is described here all the same, so that the roles have one definition.)
// Plain constexpr C++: a host program includes this file and compares every field with the formulas written out lane
// by lane (tests/test_bc7_lane_roles.py).
#ifndef CFHIP_BC7_ROLES_H
#define CFHIP_BC7_ROLES_H

#include <stdint.h>

// Layouts.  Low walks Normal's candidate set, High Highest's: the level's budget is not part of a role.
#define CF_ROLE_LAY_LOWEST 0u   // 32 lanes per block: mode 6, mode 5 rotation 0 (blocks with alpha)
#define CF_ROLE_LAY_NORMAL 1u   // 32 lanes per block: + the rotations of mode 5, modes 1 / 3 or 7; second pass 0 / 2 or 4
#define CF_ROLE_LAY_WIDE 2u     // 64 lanes per block: + mode 4, 16 two-subset slots; second pass modes 0 / 2

// Role word.
//   bits  0..3   kind, one bit each: mode 6, vector plane, scalar plane, partition subset (0: the lane has no role)
//   bits  4..12  candidate id (mode 6, planes) or the id of partition 0 of the lane's mode (subsets: + the partition)
//   bits 13..14  fit index of the lane inside its candidate: subset, 1 for a scalar plane
//   bit  15      mi: the subset's slot belongs to the second mode of the trip (3 after 1, 2 after 0)
//   bits 16..20  rank of the slot among its mode's partitions; CF_ROLE_NO_RANK on every lane that is no subset
//   bit  21      the lane leads its candidate: the candidate's fits are gathered into its column
//                (with `active`: an inactive lane leads nothing)
//   bit  22      use1: the fit of lane + 1 belongs to the leader's candidate (subset 1)
//   bit  23      use2: the fit of lane s2 does (scalar plane, subset 2)
//   bits 24..29  s2 as a lane of the half; 0 where the leader gathers nothing from it
//   bit  30      active: the lane runs a fit (linear metric)
//   bit  31      active under the perceptual metric, which splits no colour channel off (rotation 0 only)
// s1 is lane + 1 in every layout and is not stored.
#define CF_ROLE_M6 1u
#define CF_ROLE_VECP 2u
#define CF_ROLE_SCA 4u
#define CF_ROLE_PLANE 8u
#define CF_ROLE_IDB(w) (((w) >> 4) & 511u)
#define CF_ROLE_KF(w) (((w) >> 13) & 3u)
#define CF_ROLE_RANKMI(w) (((w) >> 15) & 63u)   /* mi | rank << 1: what phase 1 compares with (selection << 1 | run) */
#define CF_ROLE_NO_RANK 31u
#define CF_ROLE_LEADER(w) (((w) >> 21) & 1u)
#define CF_ROLE_USE1(w) (((w) >> 22) & 1u)
#define CF_ROLE_USE2(w) (((w) >> 23) & 1u)
#define CF_ROLE_S2(w) (((w) >> 24) & 63u)
#define CF_ROLE_ACTIVE(w, unitw) (((w) >> ((unitw) ? 30u : 31u)) & 1u)

// Fit word: the fit's static arguments.
//   bits  0..1   rot
//   bits  2..17  cb | ab << 4 | pbk << 8 | ib << 12 (fit_lane's `geo` packing)
//   bits 18..21  chm: the channels the fit codes, after rotation
#define CF_FIT_ROT(w) ((w) & 3u)
#define CF_FIT_GEO(w) (((w) >> 2) & 0xFFFFu)
#define CF_FIT_CHM(w) (((w) >> 18) & 15u)

struct cf_bc7_lane_role {
	uint32_t kind, idb, kf, mi, rank;
	bool leader, use1, use2, active, active_perceptual;
	uint32_t s2;
	uint32_t rot, cb, ab, pbk, ib, chm;
};

// The role of lane hl of a half.  st: 0 first pass, 1 second.  alpha: the half's block carries alpha.  gate: the half
// walks the second pass (read in the second pass of the 32-lane layouts alone).
constexpr cf_bc7_lane_role cf_bc7_role(uint32_t lay, uint32_t st, bool alpha, bool gate, uint32_t hl)
{
	cf_bc7_lane_role r = {0u, 0u, 0u, 0u, CF_ROLE_NO_RANK, false, false, false, false, false, 0u,
		0u, 7u, 7u, 1u, 4u, alpha ? 15u : 7u};
	const bool wide = lay == CF_ROLE_LAY_WIDE, normal = lay == CF_ROLE_LAY_NORMAL;
	uint32_t nplanes = 0, plane0 = 2;      // vector planes from lane plane0, their scalar planes nplanes lanes up
	uint32_t cid0 = 1, slot = 0;
	uint32_t pfirst = 0, nslots = 0, ns = 2u + st, nper0 = 0, id0 = 0, id1 = 0;
	if (st == 0u) {
		nplanes = wide ? 12u : (normal ? 4u : 1u);
		pfirst = wide ? 26u : 10u;
		nslots = wide ? 16u : (normal ? 11u : 0u);
		nper0 = alpha ? nslots : (wide ? 12u : 6u);
		id0 = alpha ? 320u : 64u; id1 = 128u;
		if (hl < 2u) {
			r.kind = CF_ROLE_M6; r.leader = hl == 0u; r.active = r.active_perceptual = true; r.chm = 15u;
			return r;
		}
	} else if (wide) {
		nslots = 10u; nper0 = 5u; id0 = 192u; id1 = 256u;
	} else if (gate && alpha) {
		// mode 4 of an alpha-carrying half: candidate 5 + k in lanes 11 + 2 k (vector plane), 12 + 2 k (scalar plane)
		if (hl >= 11u && hl < 27u) {
			const uint32_t k = (hl - 11u) >> 1;
			const bool sca = ((hl - 11u) & 1u) != 0u;
			const uint32_t cid = 5u + k, isel = k >> 2;
			r.kind = sca ? CF_ROLE_SCA : CF_ROLE_VECP;
			r.idb = cid; r.kf = sca ? 1u : 0u;
			r.rot = k & 3u; r.pbk = 0u;
			r.cb = sca ? 0u : 5u; r.ab = sca ? 6u : 0u;
			r.ib = (isel != 0u) == sca ? 2u : 3u;
			r.chm = sca ? 8u : 7u;
			r.active = normal; r.active_perceptual = normal && r.rot == 0u;
			r.leader = !sca && r.active; r.use2 = !sca; r.s2 = sca ? 0u : hl + 1u;
		}
		return r;
	} else if (gate && normal) {
		// modes 0 / 2 of an opaque half: slot s has its subsets in lanes 11 + 2 s, 12 + 2 s and s
		if (hl != 10u && hl != 31u) {
			slot = hl < 10u ? hl : (hl - 11u) >> 1;
			r.kf = hl < 10u ? 2u : (hl - 11u) & 1u;
			r.mi = slot >= 5u ? 1u : 0u;
			r.rank = slot - 5u*r.mi;
			r.kind = CF_ROLE_PLANE; r.idb = r.mi ? 256u : 192u;
			r.cb = r.mi ? 5u : 4u; r.ab = 0u; r.pbk = r.mi ? 0u : 1u; r.ib = r.mi ? 2u : 3u;
			r.active = r.active_perceptual = true;
			r.leader = r.kf == 0u; r.use1 = r.use2 = true; r.s2 = r.leader ? slot : 0u;
		}
		return r;
	} else
		return r;
	// planes of modes 5 / 4 (first pass)
	if (nplanes && hl >= plane0 && hl < plane0 + 2u*nplanes) {
		const bool sca = hl >= plane0 + nplanes;
		const uint32_t cid = cid0 + (hl - plane0) - (sca ? nplanes : 0u);
		r.kind = sca ? CF_ROLE_SCA : CF_ROLE_VECP;
		r.idb = cid; r.kf = sca ? 1u : 0u; r.pbk = 0u;
		if (cid <= 4u) {
			r.rot = cid - 1u; r.ib = 2u;
			r.cb = sca ? 0u : 7u; r.ab = sca ? 8u : 0u;
			r.active = (normal || wide) ? true : alpha;
		} else {
			const uint32_t isel = (cid - 5u) >> 2;
			r.rot = (cid - 5u) & 3u;
			r.cb = sca ? 0u : 5u; r.ab = sca ? 6u : 0u;
			r.ib = (isel != 0u) == sca ? 2u : 3u;
			r.active = true;
		}
		r.active_perceptual = r.active && r.rot == 0u;
		r.chm = sca ? 8u : 7u;
		r.leader = !sca && r.active; r.use2 = !sca; r.s2 = sca ? 0u : hl + nplanes;
		return r;
	}
	// partition subsets in consecutive lanes from pfirst
	if (hl >= pfirst && (hl - pfirst)/ns < nslots) {
		slot = (hl - pfirst)/ns;
		r.kf = (hl - pfirst) - slot*ns;
		r.mi = slot >= nper0 ? 1u : 0u;
		r.rank = slot - r.mi*nper0;
		r.kind = CF_ROLE_PLANE; r.idb = r.mi ? id1 : id0;
		const uint32_t mode = st ? (r.mi ? 2u : 0u) : (alpha ? 7u : (r.mi ? 3u : 1u));
		r.cb = (0x57757564u >> (4u*mode)) & 15u; r.ab = (0x57860000u >> (4u*mode)) & 15u;
		r.pbk = (0x11001021u >> (4u*mode)) & 15u; r.ib = (0x24222233u >> (4u*mode)) & 15u;
		r.active = r.active_perceptual = true;
		r.leader = r.kf == 0u; r.use1 = true; r.use2 = st == 1u; r.s2 = (r.leader && r.use2) ? hl + 2u : 0u;
	}
	return r;
}

constexpr uint32_t cf_bc7_role_word(uint32_t lay, uint32_t st, bool alpha, bool gate, uint32_t hl)
{
	const cf_bc7_lane_role r = cf_bc7_role(lay, st, alpha, gate, hl);
	return r.kind | (r.idb << 4) | (r.kf << 13) | (r.mi << 15) | (r.rank << 16) | ((r.leader ? 1u : 0u) << 21) |
		((r.use1 ? 1u : 0u) << 22) | ((r.use2 ? 1u : 0u) << 23) | (r.s2 << 24) | ((r.active ? 1u : 0u) << 30) |
		((r.active_perceptual ? 1u : 0u) << 31);
}

constexpr uint32_t cf_bc7_fit_word(uint32_t lay, uint32_t st, bool alpha, bool gate, uint32_t hl)
{
	const cf_bc7_lane_role r = cf_bc7_role(lay, st, alpha, gate, hl);
	return r.rot | ((r.cb | (r.ab << 4) | (r.pbk << 8) | (r.ib << 12)) << 2) | (r.chm << 18);
}

// The table: per layout and row, per lane, the role word and the fit word.
// 32-lane layouts: [layout][row][hl].  Rows 0 / 1: first pass of an opaque / alpha-carrying half; 2 / 3: second pass of
// an opaque / alpha-carrying half that walks it; 4: a half without roles (it does not walk the second pass, or the wave
// holds one block and these are its upper lanes).  64-lane layout, after them: [row][lane], rows 0 / 1 as above, row 2
// the second pass (opaque blocks only; the wave walks it or skips the trip).
#define CF_ROLE_ROWS 5u
#define CF_ROLE_ROW_NONE 4u
#define CF_ROLE_WIDE_ROWS 3u
#define CF_ROLE_WIDE_BASE (2u*CF_ROLE_ROWS*32u*2u)
struct cf_bc7_role_table { uint32_t w[CF_ROLE_WIDE_BASE + CF_ROLE_WIDE_ROWS*64u*2u]; };
constexpr uint32_t cf_bc7_role_index(uint32_t lay, uint32_t row, uint32_t hl)
{
	return lay == CF_ROLE_LAY_WIDE ? CF_ROLE_WIDE_BASE + (row*64u + hl)*2u : ((lay*CF_ROLE_ROWS + row)*32u + hl)*2u;
}
constexpr cf_bc7_role_table cf_bc7_make_roles()
{
	cf_bc7_role_table t = {};
	for (uint32_t lay = 0; lay < 3u; ++lay) {
		const bool wide = lay == CF_ROLE_LAY_WIDE;
		for (uint32_t row = 0; row < (wide ? CF_ROLE_WIDE_ROWS : CF_ROLE_ROWS); ++row)
			for (uint32_t hl = 0; hl < (wide ? 64u : 32u); ++hl) {
				const uint32_t st = row >= 2u ? 1u : 0u;
				const bool alpha = row == 1u || row == 3u, gate = row == 2u || row == 3u;
				const uint32_t i = cf_bc7_role_index(lay, row, hl);
				t.w[i] = cf_bc7_role_word(lay, st, alpha, gate, hl);
				t.w[i + 1u] = cf_bc7_fit_word(lay, st, alpha, gate, hl);
			}
	}
	return t;
}

#endif
