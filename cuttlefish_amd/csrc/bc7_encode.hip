// bc7_encode.hip -- BC7 block encoder for gfx950 (MI355X), one wavefront per block.
//
// Replaces, behind cfhip_encode(), the per-block call the reference makes in
// Bc7Converter::compressBlock (lib/src/S3tcConverter.cpp:632-646) into
// bc7enc_compress_block / ispc::bc7e_compress_blocks(1, ...), with the per-quality
// budgets of createBc7BlockParams (S3tcConverter.cpp:170-227).
//
// Mapping:
//   * workgroup = 4 wave64 = a strip of 16 adjacent blocks; the tile and a channel-planar
//     copy of it are staged in LDS by coalesced row loads (cf_device.h).
//   * the kernel is VALU-issue-bound and an instruction costs the same whatever the number
//     of active lanes, so ONE fit per lane and ONE instruction stream: mode, rotation, channel
//     set, precision, p-bit kind, index width and subset mask are per-lane values (fit_lane:
//     integer statistics -> covariance -> principal axis -> extremes -> quantise -> exhaustive
//     selectors via v_dot4_u32_u8 -> closed-form least-squares refit rounds).
//   * what a lane fits in a stream trip -- its role -- depends on the layout, the trip, whether its half carries alpha
//     and walks the second pass, and its index in the half, on nothing the search computes: two packed words per lane
//     (kind, candidate id, fit index, rank, leader and gather flags; rotation, precisions, channel set) from a table
//     built at compile time (bc7_roles.h).  They are loaded before the fit and again after it, so no role lives in a
//     register through the fit, and the candidate assembly after the fit is straight-line code under one guard.
//     (Lowest keeps its roles as expressions: four lanes with a role fold to constants, and the words did not pay.)
//   * up to High a block's candidates fill 32 lanes (mode 6, mode 5 x rotations, modes 1/3
//     or 7 on their best partitions) and two neighbouring blocks share a wavefront; Highest uses
//     64 lanes (mode 4, 16 two-subset partitions) and a second stream for the three-subset modes.
//   * High / Highest then perturb the winner ("uber" levels of bc7enc, S3tcConverter.cpp:200-215):
//     lane = (fit of the winner, one of 16 +-1 endpoint / p-bit moves), exact error by the same
//     selector assignment, best move per fit per round -- the extra work is extra LANES of one
//     more assignment pass, not extra candidates walked in sequence.
//   * partitions are ranked once per subset count by a residual estimator (subset_residual)
//     and the best are taken by an iterated group minimum (DPP rows + v_readlane).
//   * all error arithmetic is integer; a lane keeps (error, id) in registers and its best
//     candidate's fields in its LDS column; group argmin on (error, id); the whole group then
//     bit-packs the winner (one bit field per lane, OR-reduced), written out coalesced via LDS.
//   * the search is integer and float VALU work (roofline in DESIGN.md section 4) with one use of the matrix pipe: under unit
//     weights the selector search takes the cross terms of a row of four texels against a palette entry from one
//     v_mfma_i32_4x4x4_16b_i8, for which the fit runs with the whole wave on; the perceptual metric's are v_dot2_u32_u16 pairs.
//
// Candidate ids and every float operation order are identical to the CPU oracle
// (oracle/bc7_encode.c), so the payload is byte-identical to it.
// Build with -ffp-contract=off: fused ops are written as explicit fmaf().
#include "cf_device.h"
#include "bc7_packed.h"
#include "bc7_rcp.h"
#include "bc7_roles.h"
#include "bc7_cand.h"
#include "bc7_pack.h"

namespace {

// the lane id, recomputed where a phase starts: a volatile mbcnt pair cannot be hoisted or merged, so no
// lane-derived value has to stay in a register (or be spilled) across the phases of the search
#define CF_FRESH_LANE(x) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(x))

// value of lane `src` (mod 64): ds_bpermute without the lane-id arithmetic __shfl wraps around it (a
// hoisted mbcnt pair is one more VGPR alive through the whole search)
__device__ __forceinline__ int cf_bperm(int v, uint32_t src)
{
	return __builtin_amdgcn_ds_bpermute((int)(src << 2), v);
}

// what every lane of a stream trip does, as two words per (layout, row, lane): bc7_roles.h
__device__ const cf_bc7_role_table k_bc7_roles = cf_bc7_make_roles();

// what a stored candidate is, by id, and the texels of its fits (bc7_cand.h)
__device__ const cf_bc7_cand_table k_bc7_cands = cf_bc7_make_cands();
__device__ const cf_bc7_mask_table k_bc7_masks = cf_bc7_make_masks();
__device__ const cf_bc7_pack_table k_bc7_pack = cf_bc7_make_pack();

// the interpolation weights of a fit's palette entries as bytes (bc7_packed.h)
__device__ const cf_bc7_weight_table k_bc7_weights = cf_bc7_make_weights();

__device__ const uint16_t k_part2[64] = CF_BC7_PART2_INIT;

__device__ const uint8_t k_anchor2[64] = {
	15,15,15,15,15,15,15,15, 15,15,15,15,15,15,15,15,
	15, 2, 8, 2, 2, 8, 8,15,  2, 8, 2, 2, 8, 8, 2, 2,
	15,15, 6, 8, 2, 8,15,15,  2, 8, 2, 2, 2,15,15, 6,
	 6, 2, 6, 8,15,15, 2, 2, 15,15,15,15,15, 2, 2,15
};

__device__ const uint32_t k_part3[64] = CF_BC7_PART3_INIT;

__device__ const uint8_t k_anchor3a[64] = {
	 3, 3,15,15, 8, 3,15,15,  8, 8, 6, 6, 6, 5, 3, 3,
	 3, 3, 8,15, 3, 3, 6,10,  5, 8, 8, 6, 8, 5,15,15,
	 8,15, 3, 5, 6,10, 8,15, 15, 3,15, 5,15,15,15,15,
	 3,15, 5, 5, 5, 8, 5,10,  5,10, 8,13,15,12, 3, 3
};

__device__ const uint8_t k_anchor3b[64] = {
	15, 8, 8, 3,15,15, 3, 8, 15,15,15,15,15,15,15, 8,
	15, 8,15, 3,15, 8,15, 8,  3,15, 6,10,15,15,10, 8,
	15, 3,15,10,10, 8, 9,10,  6,15, 8,15, 3, 6, 6, 8,
	15, 3,15,15,15,15,15,15, 15,15,15,15, 3,15,15, 8
};

// Texels of subset sb of a three-subset partition word (2 bits per texel): the texels whose pair equals sb as
// bits at the even positions, then the even bits squeezed into the low half.
__device__ __forceinline__ uint32_t part3_mask(uint32_t p3, uint32_t sb)
{
	const uint32_t lo = p3 & 0x55555555u, hi = (p3 >> 1) & 0x55555555u;
	uint32_t x = sb == 0u ? ~(lo | hi) & 0x55555555u : (sb == 1u ? lo & ~hi : (sb == 2u ? hi & ~lo : 0u));
	x = (x | (x >> 1)) & 0x33333333u;
	x = (x | (x >> 2)) & 0x0F0F0F0Fu;
	x = (x | (x >> 4)) & 0x00FF00FFu;
	return (x | (x >> 8)) & 0xFFFFu;
}

struct SubFit {
	uint32_t e0, e1;   // dequantised endpoints, bytes r,g,b,a
	uint32_t q0, q1;   // quantised fields, bytes r,g,b,a
	uint32_t pb;       // bit0: p-bit of endpoint 0, bit1: endpoint 1
	uint32_t err;
	uint32_t w[4];     // interpolation weight per pixel (bytes), 0 outside the subset
	float nx0[4], nx1[4];   // least-squares endpoints for these selectors (next round)
	bool ok;                // least-squares system was solvable
};

struct Cand {
	uint32_t err, id;
	uint32_t q[6];     // q[2s+e]
	uint32_t pb;       // bit 2s+e
	uint32_t w[4];     // vector-plane weights per pixel
	uint32_t w2[4];    // scalar-plane weights per pixel (modes 4/5)
};

// A lane's best candidate so far lives in LDS (field-major, one column per thread):
// only (error, id) stay in registers.  22 words: q[6], pb, w[4], w2[4], the errors of its (up to
// three) fits -- what the refinement of the best candidates compares against -- and four words where
// (error, id) and the lanes of the (up to eight) best candidates are parked while the lane runs another fit.
#define CF_BC7_CAND_WORDS 22
__device__ __forceinline__ void cand_store(uint32_t* slot, const Cand& c)
{
#pragma unroll
	for (int k = 0; k < 6; ++k) slot[k*CF_WG_THREADS] = c.q[k];
	slot[6*CF_WG_THREADS] = c.pb;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		slot[(7 + k)*CF_WG_THREADS] = c.w[k];
		slot[(11 + k)*CF_WG_THREADS] = c.w2[k];
	}
}

__device__ __forceinline__ uint32_t ub(uint32_t v, int c) { return (v >> (8*c)) & 255u; }
__device__ __forceinline__ float fb(uint32_t v, int c) { return (float)((v >> (8*c)) & 255u); }

// One median instruction.  Equal to the two compares and selects for every finite x, but that -0.0 may come out as
// +0.0, which changes no product, floorf or difference downstream; no active lane clamps a NaN (axis, mean and extremes
// of a non-empty subset are finite, and a singular refit divides by 64).
__device__ __forceinline__ float clamp255(float x)
{
	return __builtin_amdgcn_fmed3f(x, 0.0f, 255.0f);
}

// 1/n of a subset of n = 1..16 texels: the correctly rounded quotients as literals, the same floats as the
// division gives (which the compiler expands to the full IEEE sequence, ~10 instructions, for a per-lane n).
// Entry 0 keeps the division's result for a lane that carries no subset.
__device__ const float k_inv_n[17] = {
	__builtin_huge_valf(), 1.0f/1.0f, 1.0f/2.0f, 1.0f/3.0f, 1.0f/4.0f, 1.0f/5.0f, 1.0f/6.0f, 1.0f/7.0f, 1.0f/8.0f,
	1.0f/9.0f, 1.0f/10.0f, 1.0f/11.0f, 1.0f/12.0f, 1.0f/13.0f, 1.0f/14.0f, 1.0f/15.0f, 1.0f/16.0f
};
__device__ __forceinline__ float inv_n(uint32_t n) { return k_inv_n[n < 16u ? n : 16u]; }

// (2^t - 1)/255 for a per-lane t: a select chain on literals instead of a table load
// (a divergent index would make it a vector memory load on the critical path).
__device__ __forceinline__ float sc_of(uint32_t t)
{
	float r = 0.0f/255.0f;
	r = t == 4u ? 15.0f/255.0f : r;
	r = t == 5u ? 31.0f/255.0f : r;
	r = t == 6u ? 63.0f/255.0f : r;
	r = t == 7u ? 127.0f/255.0f : r;
	r = t == 8u ? 255.0f/255.0f : r;
	return r;
}

// C: quantise float endpoints.  cb: bits of channels 0..2, ab: bits of channel 3
// (0 = channel not coded).  pbk: 0 none, 1 per endpoint, 2 shared.  All may differ per lane,
// so there is ONE straight-line path: both p-bit candidates of both endpoints are formed as
//   q = clamp(floor((x*sc(T) - P)*H + 0.5)),  code = (q << S) | P,  d = dequant(code, T)
// with (T, H, S) = (bits+1, 0.5, 1) for p-bit modes and (bits, 1.0, 0) with P forced to 0
// otherwise -- for those lanes (y - 0)*1 is exact, both candidates coincide and p = 0 wins.
// A channel that is not coded has x = 0 and comes out as 0 (its dequantised pattern is masked).
// UNITW: every coded channel weighs 1 and a channel that is not coded contributes an exact zero, so the
// weights need no registers (fmaf(1, t2, acc) is the same correctly rounded sum as the oracle's).
template <bool UNITW>
__device__ __forceinline__ void quantize(const float (&x0)[4], const float (&x1)[4], uint32_t cb,
	uint32_t ab, uint32_t pbk, const uint32_t (&wt)[4], SubFit& f)
{
	const uint32_t S = pbk ? 1u : 0u;
	const float H = pbk ? 0.5f : 1.0f;
	const uint32_t Tc = cb + S, Ta = ab + S;
	const float scc = cb ? sc_of(Tc) : 0.0f, sca = ab ? sc_of(Ta) : 0.0f;
	const float qmc = (float)((1 << cb) - 1), qma = (float)((1 << ab) - 1);
	const uint32_t tc = cb ? Tc : 0u, ta = ab ? Ta : 0u;
	// [endpoint][p]: the fields and the dequantised bytes as whole words (bc7_packed.h)
	uint32_t q[2][2], d[2][2];
	float er[2][2];
#pragma unroll
	for (int e = 0; e < 2; ++e) {
#pragma unroll
		for (int p = 0; p < 2; ++p) {
			const uint32_t P = pbk ? (uint32_t)p : 0u;
			const float Pf = (float)P;
			uint32_t qw = 0;
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				const float sc = c < 3 ? scc : sca;
				const float xv = e ? x1[c] : x0[c];
				const float y = xv*sc;
				const float u = (y - Pf)*H;
				// clamped as a float (an integer below 256 either way), converted and inserted as byte c in one instruction
				const float r = __builtin_amdgcn_fmed3f(floorf(u + 0.5f), 0.0f, c < 3 ? qmc : qma);
				qw = __builtin_amdgcn_cvt_pk_u8_f32(r, (uint32_t)c, qw);
			}
			const uint32_t dw = dequant_word(code_word(qw, S, P), tc, ta);
			float acc = 0.0f;
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				const float xv = e ? x1[c] : x0[c];
				const float dx = fb(dw, c) - xv;
				const float t2 = dx*dx;
				acc = UNITW ? acc + t2 : fmaf((float)wt[c], t2, acc);
			}
			q[e][p] = qw;
			d[e][p] = dw;
			er[e][p] = acc;
		}
	}
	uint32_t p0, p1;
	{
		const uint32_t i0 = er[0][1] < er[0][0] ? 1u : 0u;
		const uint32_t i1 = er[1][1] < er[1][0] ? 1u : 0u;
		const float s0 = er[0][0] + er[1][0];
		const float s1 = er[0][1] + er[1][1];
		const uint32_t sh = s1 < s0 ? 1u : 0u;
		p0 = pbk == 1u ? i0 : (pbk == 2u ? sh : 0u);
		p1 = pbk == 1u ? i1 : (pbk == 2u ? sh : 0u);
	}
	f.q0 = p0 ? q[0][1] : q[0][0];
	f.e0 = p0 ? d[0][1] : d[0][0];
	f.q1 = p1 ? q[1][1] : q[1][0];
	f.e1 = p1 ? d[1][1] : d[1][0];
	f.pb = p0 | (p1 << 1);
}

// View of one block's texels in LDS for one fit: packed RGBA words (tp) and the
// channel-planar copy (pl: row r -> 4 words R,G,B,A, texel j of the row in byte j),
// the lane's channel rotation and the set of (rotated) channels this fit codes.
struct Tex {
	// the workgroup's three LDS arrays (compile-time addresses once inlined) and ONE per-lane value, the
	// block's word offset: the three per-block pointers are expressions of it, not three live registers
	const uint32_t* tile_;
	const uint32_t* plan_;
	const uint32_t* yccp_; // perceptual metric only: the texels as (Y | Cr << 16, Cb | A << 16) word pairs
	uint32_t boff;         // block index x 16
	__device__ __forceinline__ const uint32_t* tp() const { return tile_ + boff; }
	__device__ __forceinline__ const uint32_t* pl() const { return plan_ + boff; }
	__device__ __forceinline__ const uint32_t* yc() const { return yccp_ + 2u*boff; }
	uint32_t sel;      // v_perm_b32 selector of the rotation; 0x0C (a zero byte) for a channel that is not coded
	uint32_t rot;      // 0..3
	uint32_t chmask;   // bit c: rotated channel c is coded by this fit
	uint32_t vmask;    // byte mask of chmask
};

__device__ __forceinline__ Tex make_tex(const uint32_t* tile, const uint32_t* plan, const uint32_t* yccp, uint32_t boff,
	uint32_t rot, uint32_t chmask)
{
	Tex t;
	t.tile_ = tile; t.plan_ = plan; t.yccp_ = yccp; t.boff = boff; t.rot = rot; t.chmask = chmask;
	const uint32_t sel = rot == 0u ? 0x03020100u : (rot == 1u ? 0x00020103u :
		(rot == 2u ? 0x01020300u : 0x02030100u));
	t.vmask = ((chmask & 1u) ? 0xFFu : 0u) | ((chmask & 2u) ? 0xFF00u : 0u) |
		((chmask & 4u) ? 0xFF0000u : 0u) | ((chmask & 8u) ? 0xFF000000u : 0u);
	t.sel = (sel & t.vmask) | (0x0C0C0C0Cu & ~t.vmask);
	return t;
}

template <bool ROT>
__device__ __forceinline__ uint32_t texel(const Tex& t, uint32_t raw)
{
	// rotated: the selector already zeroes the channels that are not coded
	return ROT ? __builtin_amdgcn_perm(raw, raw, t.sel) : raw & t.vmask;
}

// The four channel planes of one texel row after rotation, non-coded channels zeroed.
template <bool ROT>
__device__ __forceinline__ void planes(const Tex& t, const uint4 pr, uint32_t (&P)[4])
{
	if (ROT) {
		P[0] = t.rot == 1u ? pr.w : pr.x;
		P[1] = t.rot == 2u ? pr.w : pr.y;
		P[2] = t.rot == 3u ? pr.w : pr.z;
		P[3] = t.rot == 0u ? pr.w : (t.rot == 1u ? pr.x : (t.rot == 2u ? pr.y : pr.z));
	} else {
		P[0] = pr.x; P[1] = pr.y; P[2] = pr.z; P[3] = pr.w;
	}
#pragma unroll
	for (int c = 0; c < 4; ++c)
		P[c] = ((t.chmask >> c) & 1u) ? P[c] : 0u;
}

// 4 mask bits -> 4 mask bytes (0x00 / 0xFF)
__device__ __forceinline__ uint32_t bytemask4(uint32_t m)
{
	return ((m*0x00204081u) & 0x01010101u)*0xFFu;
}

// ---------------------------------------------------------------------------
// One fit per lane.  Every VALU instruction costs the wave the same issue time whatever
// the number of active lanes (tools/ubench/valu_rate.hip: 4 cycles per integer
// wave-instruction, 2 for fp32 fma/mul/add), so the cheapest schedule is the one where
// every lane carries a different fit through ONE instruction stream: all of mode, rotation,
// channel set, endpoint precision, p-bit kind, index width and subset mask are per-lane
// values here.  Mode 6 alone is spread over a lane pair (16 palette entries, 8 per lane;
// the per-texel keys meet through a DPP lane^1 exchange).  Same arithmetic as
// the oracle's fit_subset / fit_scalar.

// ---- perceptual metric (UNITW = false; oracle: to_ycc / assign) ----
// sRGB images at >= Normal ask for bc7enc's perceptual error (S3tcConverter.cpp:196-199): texels and
// palette colours are compared in (Y, Cr, Cb, A), Y = (109 R + 366 G + 37 B + 256) >> 9,
// Cr = R - Y + 255, Cb = B - Y + 255, with axis weights 16, 8, 2, 1.  Values fit 16 bits, so a texel
// is two words of 16-bit pairs and sum_ax w_ax p_ax q_ax is two chained v_dot2_u32_u16.  A fit's
// weight pair yw carries its channel set: zero weights on the axes it does not code.
typedef unsigned short cf_us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_mul_u16(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, (cf_us2)(__builtin_bit_cast(cf_us2, a)*__builtin_bit_cast(cf_us2, b)));
}

__device__ __forceinline__ uint32_t dot2_u16(uint32_t a, uint32_t b, uint32_t acc)
{
	return __builtin_amdgcn_udot2(__builtin_bit_cast(cf_us2, a), __builtin_bit_cast(cf_us2, b), acc, false);
}

__device__ __forceinline__ void ycc_pairs(uint32_t r, uint32_t g, uint32_t b, uint32_t a, uint32_t& prg, uint32_t& pba)
{
	const uint32_t y = (109u*r + 366u*g + 37u*b + 256u) >> 9;
	prg = y | ((r + 255u - y) << 16);
	pba = (b + 255u - y) | (a << 16);
}

// sum over the texels of mask of sum_ax w_ax p_ax^2: the constant part of a fit's error
__device__ __forceinline__ uint32_t ycc_pp_sum(const Tex& tx, uint32_t mask, const uint32_t (&yw)[2])
{
	uint32_t pp = 0;
#pragma unroll 1
	for (uint32_t r = 0; r < 4u; ++r) {
		const uint4 ya = *reinterpret_cast<const uint4*>(tx.yc() + 8u*r);
		const uint4 yb = *reinterpret_cast<const uint4*>(tx.yc() + 8u*r + 4u);
		const uint32_t pr[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const uint32_t t = dot2_u16(pk_mul_u16(pr[2*j], yw[0]), pr[2*j], dot2_u16(pk_mul_u16(pr[2*j + 1], yw[1]), pr[2*j + 1], 0u));
			pp += ((mask >> (4u*r + (uint32_t)j)) & 1u) ? t : 0u;
		}
	}
	return pp;
}

// Timing-ablation switches for tools/ab_build.sh (never set in the product build; every bit changes the payload):
//    1: stream fits of mode 6 and the two-plane modes only    2: no two-plane fits    4: one block per wave at every level
//    8: no refit_window   16: no starts trips   32: no perturbation rounds
#ifndef CF_BC7_ABLATE
#define CF_BC7_ABLATE 0
#endif

// Diagnostic counters (never set in the product build): per wave pass, how often the starts trip reads the
// fit-geometry cache, how often the starts trip / the perturbation pass have only fits of <= 4 palette entries, how
// often they have no fit with p-bits, and how often the perturbation pass finds pp_sum in the cache.
// Read by cfhip_bc7_diag() below.
#ifndef CF_BC7_DIAG
#define CF_BC7_DIAG 0
#endif
#if CF_BC7_DIAG
enum { CF_DIAG_STARTS, CF_DIAG_STARTS_CACHED, CF_DIAG_STARTS_NARROW, CF_DIAG_PERTURB, CF_DIAG_PERTURB_NARROW,
	CF_DIAG_STARTS_NOPB, CF_DIAG_PERTURB_NOPB, CF_DIAG_PERTURB_PPHIT, CF_DIAG_N };
__device__ unsigned long long cf_bc7_diag[CF_DIAG_N];
#define CF_DIAG_COUNT(i, cond) do { uint32_t l_; CF_FRESH_LANE(l_); if (l_ == 0u && (cond)) atomicAdd(&cf_bc7_diag[i], 1ull); } while (0)
#else
#define CF_DIAG_COUNT(i, cond) do { } while (0)
#endif

typedef int cf_int4 __attribute__((ext_vector_type(4)));
// The A operand of the matrix-pipe cross terms (assign_lsq_lane): texel (row r, column lane & 3) of block boff, bit 7 of
// every byte flipped.  Zeros under the perceptual metric, whose search does not use it.
template <bool UNITW>
__device__ __forceinline__ void arow_load(const uint32_t* tile, uint32_t boff, uint32_t (&arow)[4])
{
	arow[0] = arow[1] = arow[2] = arow[3] = 0u;
	if (UNITW) {
		uint32_t lane;
		CF_FRESH_LANE(lane);
#pragma unroll
		for (uint32_t r = 0; r < 4u; ++r)
			arow[r] = tile[boff + 4u*r + (lane & 3u)] ^ 0x80808080u;
	}
}

struct LaneFit {
	uint32_t q0, q1, pb, err;   // (the dequantised endpoints are an input of the assignment, not part of a result)
	uint32_t w[4];          // weights per texel (bytes), 0 outside the subset
};

// NK: palette entries walked per lane -- 8, or 4 when no lane of the wave has more than 4 (index width 2, not mode 6):
// entries 4..7 then carry the never-winning key and dropping them changes no minimum.
// arow (unit weights): the A operand of the matrix-pipe cross terms, words r = 0..3: texel (row r, column lane & 3)
// of the lane's block xored with 0x80808080, loaded by the caller where the whole wave is on (arow_load); CBSZ: 3 in the
// 32-lane layouts (one block per half-wavefront), 4 in the wide one.
template <bool UNITW, int NK = 8, int CBSZ = 3>
__device__ __forceinline__ void assign_lsq_lane(const Tex& tx, uint32_t mask, bool m6,
	uint32_t khalf, uint32_t ib, const uint32_t (&yw)[2], uint32_t pp_sum, bool want_lsq, uint32_t fe0, uint32_t fe1, const uint32_t (&arow)[4],
	LaneFit& f, float (&nx0)[4], float (&nx1)[4], float (&hq)[3], bool& ok, uint32_t s01 = 0u, uint32_t s23 = 0u)   // s01, s23: want_lsq only
{
	// the weight's bits below the error part of a key (bc7_packed.h): a full byte under unit weights, where a row's weights
	// leave their keys by byte permutes; 7 under the perceptual metric
	constexpr int WBITS = UNITW ? 8 : 7;
	const uint32_t nk = m6 ? 8u : (1u << ib);
	const uint32_t e00 = ub(fe0, 0), e01 = ub(fe0, 1), e02 = ub(fe0, 2), e03 = ub(fe0, 3);
	const uint32_t e10 = ub(fe1, 0), e11 = ub(fe1, 1), e12 = ub(fe1, 2), e13 = ub(fe1, 3);
	// straight-line palette: entries past this lane's 2^ib get a key that never wins.
	// A texel's key is F/2 (sum_c w_c c_k^2 - 2 sum_c p_c (w_c c_k)) + weight_k with F = 2^(WBITS + 1), minimised over k;
	// sum_c w_c p_c^2 is added once per subset (pp_sum).  Unit weights: the cross terms of a row of four texels against
	// entry k are one v_mfma_i32_4x4x4_16b_i8 (bc7_packed.h: mfma_entry_base), issued without its C operand: pp_sum comes in
	// with the texels' own term already taken off (search_pp_fold).  Perceptual metric: the palette entry goes
	// to (Y, Cr, Cb, A), its weighted form is two words of 16-bit pairs, the cross term two v_dot2_u32_u16.
	uint32_t pal[8], palh[8];
	int base[8];
	// what every entry of this fit shares: the row of weight bytes and the palette's line (bc7_packed.h)
	// (the zeros are dead, but the code generated for the refit sums below depends on their presence: a different order
	// of two v_mov_b32 and an unfused shift-add without them)
	uint32_t w03 = 0, w47 = 0;
	const uint32_t* wr = k_bc7_weights.w[weight_row(m6, khalf, ib)];
	w03 = wr[0];
	w47 = NK == 8 ? wr[1] : 0u;
	// matrix pipe: the palette in raw channel order (the rotation is a swap of two bytes, its own inverse; the slots the
	// fit does not code hold zeros in both endpoint words), so that the raw texel is the other operand
	const uint32_t rsel = tx.rot == 0u ? 0x03020100u : (tx.rot == 1u ? 0x00020103u : (tx.rot == 2u ? 0x01020300u : 0x02030100u));
	const PalLine line = pal_line(__builtin_amdgcn_perm(fe0, fe0, rsel), __builtin_amdgcn_perm(fe1, fe1, rsel));   // (unit weights only)
#pragma unroll
	for (int k = 0; k < NK; ++k) {
		// entries 0..3 exist in every fit (an index has at least two bits)
		const bool valid = k < 4 || (uint32_t)k < nk;
		// an entry past 2^ib interpolates with weight 0: its colour stays a byte vector, so the
		// dot products below stay in range and its constant keeps it from ever winning
		const uint32_t w = weight_at(w03, w47, (uint32_t)k);
		const uint32_t iw = 64u - w;
		if (UNITW) {
			// the palette in difference form: one multiply and one add per channel pair
			pal[k] = pal_at(line, w);
			palh[k] = 0;
			const int B = mfma_entry_base((int)((__builtin_amdgcn_udot4(pal[k], pal[k], 0u, false) << WBITS) | w),
				__builtin_amdgcn_udot4(pal[k], 0x01010101u, 0u, false), WBITS + 1);
			pal[k] ^= 0x80808080u;
			base[k] = valid ? B : CF_BC7_NO_ENTRY;
		} else {
			const uint32_t c0 = (__umul24(iw, e00) + __umul24(w, e10) + 32u) >> 6;
			const uint32_t c1 = (__umul24(iw, e01) + __umul24(w, e11) + 32u) >> 6;
			const uint32_t c2 = (__umul24(iw, e02) + __umul24(w, e12) + 32u) >> 6;
			const uint32_t c3 = (__umul24(iw, e03) + __umul24(w, e13) + 32u) >> 6;
			uint32_t qrg, qba;
			ycc_pairs(c0, c1, c2, c3, qrg, qba);
			// (wY Y, wCr Cr) and (wCb Cb, wA A), each <= 4080; an entry past 2^ib repeats entry 0's
			// colour with a larger constant, so it never wins
			pal[k] = pk_mul_u16(qrg, yw[0]);
			palh[k] = pk_mul_u16(qba, yw[1]);
			const uint32_t qq = dot2_u16(pal[k], qrg, dot2_u16(palh[k], qba, 0u));   // <= 3.7e6
			const int B = (int)((qq << WBITS) | w);
			base[k] = valid ? B : CF_BC7_NO_ENTRY;
		}
		// hide what base is: "base - F dt" then stays ONE v_mad_i32_i24 per entry and texel
		asm volatile("" : "+v"(base[k]));
	}
	// the key's factor -F from a scalar register (a VOP3 instruction takes no literal), opaque so that the
	// multiply is not turned back into a shift and a subtraction
	int kfac = -(2 << WBITS);
	asm volatile("" : "+s"(kfac));
	// unit weights: err sums the masked keys themselves and the error comes from that sum once per assignment
	// (bc7_packed.h: search_key_sum_error) instead of a shift and an add per texel
	uint32_t err = UNITW ? 0u : pp_sum;
	uint32_t wp0 = 0, wp1 = 0, wp2 = 0, wp3 = 0;
#pragma unroll 1
	for (uint32_t r2 = 0; r2 < 4u; r2 += 2u) {
		// two rows per trip: the four weight words then rotate by two once per trip instead of by one per row
		// (the loop-carried copies were six v_mov_b32 per row)
		uint32_t wpair[2];
#pragma unroll
		for (uint32_t h = 0; h < 2u; ++h) {
			const uint32_t r = r2 + h;
			// unit weights: the row's packed RGBA texels; perceptual: its (Y | Cr, Cb | A) word pairs
			uint32_t raw[4], rawh[4];
			if (UNITW) {
				const uint4 rw = *reinterpret_cast<const uint4*>(tx.tp() + 4u*r);
				raw[0] = rw.x; raw[1] = rw.y; raw[2] = rw.z; raw[3] = rw.w;
				rawh[0] = rawh[1] = rawh[2] = rawh[3] = 0u;
			} else {
				const uint4 ya = *reinterpret_cast<const uint4*>(tx.yc() + 8u*r);
				const uint4 yb = *reinterpret_cast<const uint4*>(tx.yc() + 8u*r + 4u);
				raw[0] = ya.x; raw[1] = ya.z; raw[2] = yb.x; raw[3] = yb.z;
				rawh[0] = ya.y; rawh[1] = ya.w; rawh[2] = yb.y; rawh[3] = yb.w;
			}
			const uint32_t mrow = (mask >> (4u*r)) & 15u;
			uint32_t wrow = 0, krow[4];
			int bestm[4] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF};
			if (UNITW) {
				// C = 0: D = sum_c a'_c b'_c for the four texels against entry k.  The texel's own term 128 sum_c a_c shifts all its
				// keys alike and is taken off pp_sum once per fit (bc7_packed.h: search_pp_fold)
				const cf_int4 cop = {0, 0, 0, 0};
				const uint32_t aop = r2 == 0u ? (h == 0u ? arow[0] : arow[1]) : (h == 0u ? arow[2] : arow[3]);
#pragma unroll
				for (int k = 0; k < NK; ++k) {
					const cf_int4 d = __builtin_amdgcn_mfma_i32_4x4x4i8((int)aop, (int)pal[k], cop, CBSZ, 0, 0);
					const int v0 = key_min_form(d.x, kfac, base[k]), v1 = key_min_form(d.y, kfac, base[k]);
					const int v2 = key_min_form(d.z, kfac, base[k]), v3 = key_min_form(d.w, kfac, base[k]);
					bestm[0] = v0 < bestm[0] ? v0 : bestm[0]; bestm[1] = v1 < bestm[1] ? v1 : bestm[1];
					bestm[2] = v2 < bestm[2] ? v2 : bestm[2]; bestm[3] = v3 < bestm[3] ? v3 : bestm[3];
				}
				// mode 6: the other palette half lives in the neighbouring lane.  Once per row, behind the row's last
				// matrix instruction and under the execution mask of the mode-6 lanes (a lane pair is on or off together):
				// four v_min_i32_dpp for the wave's few mode-6 lanes instead of an exchange and a select per texel in every
				// lane.  No matrix instruction may stand inside the masked region: it would mis-read the A rows of the
				// lanes switched off (tools/ubench/mfma_layout.hip).
				if (NK == 8) {
					if (m6) {
#pragma unroll
						for (int j = 0; j < 4; ++j) {
							const int other = (int)cf_xor1((uint32_t)bestm[j]);
							bestm[j] = other < bestm[j] ? other : bestm[j];
						}
					}
				}
			}
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				uint32_t rawj = raw[j];
				// one texel at a time: interleaving the 32 dot products of a row for ILP costs
				// ~20 registers, and the kernel is issue-bound, not latency-bound
				if (!UNITW) asm volatile("" : "+v"(rawj), "+v"(wrow));
				uint32_t key;
				{
					int bestk = bestm[j];
					const uint32_t prg = rawj, pba = rawh[j];
#pragma unroll
					for (int k = 0; k < (UNITW ? 0 : NK); ++k) {
						const int dt = (int)dot2_u16(pba, palh[k], dot2_u16(prg, pal[k], 0u));
						const int v = key_min_form(dt, kfac, base[k]);
						bestk = v < bestk ? v : bestk;
					}
					// mode 6, perceptual metric: the other palette half lives in the neighbouring lane (the 4-entry search
					// is entered only when no active lane of the wave is a mode-6 lane: it has no exchange at all)
					if (NK == 8 && !UNITW) {
						const int other = (int)cf_xor1((uint32_t)bestk);
						bestk = (m6 && other < bestk) ? other : bestk;
					}
					key = (uint32_t)bestk;   // F/2 (sum w c^2 - 2 p.(w c)) + weight, two's complement
				}
				key = ((mrow >> j) & 1u) ? key : 0u;
				err += UNITW ? key : (uint32_t)((int)key >> WBITS);
				if (UNITW) krow[j] = key;
				else wrow |= (key & 127u) << (8*j);
			}
			wpair[h] = UNITW ? key_row_weights(krow[0], krow[1], krow[2], krow[3]) : wrow;
		}
		wp0 = wp2; wp1 = wp3; wp2 = wpair[0]; wp3 = wpair[1];
	}
	if (!UNITW) f.err = err;
	f.w[0] = wp0; f.w[1] = wp1; f.w[2] = wp2; f.w[3] = wp3;
	// the refit sums in a loop of their own: their 6 accumulators and the planar rows are
	// then not live across the texel search above (which holds the 16 palette registers)
	uint32_t S = 0, A = 0, B = 0, C = 0, U[4] = {0, 0, 0, 0}, V[4] = {0, 0, 0, 0};
	// unit weights: the four trips unrolled, every weight word read where it lies (as a loop it rotated the four words
	// through four v_mov_b32 per trip); the perceptual instances keep the loop
	constexpr int SUMS_UNROLL = UNITW ? 4 : 1;
	if (want_lsq) {   // uniform: the last round's refit would never be used
#pragma unroll SUMS_UNROLL
		for (uint32_t r = 0; r < 4u; ++r) {
			const uint32_t wrow = UNITW ? f.w[r] : wp0;
			if (!UNITW) { wp0 = wp1; wp1 = wp2; wp2 = wp3; wp3 = wrow; }   // rotates back to the start after 4 trips
			uint32_t P[4];
			// (the block offset made opaque per trip: the row address is then formed here, with the array's base in
			// the instruction's offset field, instead of being hoisted into a register that lives across the search)
			uint32_t bo = tx.boff;
			asm volatile("" : "+v"(bo));
			planes<true>(tx, *reinterpret_cast<const uint4*>(tx.plan_ + bo + 4u*r), P);
			S = __builtin_amdgcn_udot4(wrow, 0x01010101u, S, false);
			C = __builtin_amdgcn_udot4(wrow, wrow, C, false);
#pragma unroll
			for (int c = 0; c < 4; ++c)
				V[c] = __builtin_amdgcn_udot4(wrow, P[c], V[c], false);
		}
		// the sums with iw = 64 - w (exact on the subset, where both are integers; w = 0 outside it) from the sums
		// with w and the subset's channel sums s_c (s01, s23: 16-bit pairs)
		A = 4096u*(uint32_t)__builtin_popcount(mask) - 128u*S + C;
		B = 64u*S - C;
		U[0] = 64u*(s01 & 0xFFFFu) - V[0]; U[1] = 64u*(s01 >> 16) - V[1];
		U[2] = 64u*(s23 & 0xFFFFu) - V[2]; U[3] = 64u*(s23 >> 16) - V[3];
	}
	if (UNITW) {
		// the weights' sum: the refit sums' S where they ran, otherwise four dot products
		uint32_t ws = S;
		if (!want_lsq)
			ws = __builtin_amdgcn_udot4(f.w[0], 0x01010101u, __builtin_amdgcn_udot4(f.w[1], 0x01010101u,
				__builtin_amdgcn_udot4(f.w[2], 0x01010101u, __builtin_amdgcn_udot4(f.w[3], 0x01010101u, 0u, false), false), false), false);
		f.err = search_key_sum_error(pp_sum, err, ws);
	}
	const int det = (int)__umul24((uint32_t)__builtin_popcount(mask), C) - (int)__umul24(S, S);
	ok = det > 0;
	const float inv = cf_rcp_ranged(64.0f*(float)(det > 0 ? det : 1));
	const float fA = (float)A, fB = (float)B, fC = (float)C;
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		if ((tx.chmask >> c) & 1u) {
			const float fU = (float)U[c], fV = (float)V[c];
			const float t0 = fB*fV;
			const float n0 = fmaf(fC, fU, -t0);
			const float t1 = fB*fU;
			const float n1 = fmaf(fA, fV, -t1);
			// UNCLAMPED: the quadratic form of refit_window is centred here; fit_lane clamps for the rounding
			nx0[c] = n0*inv;
			nx1[c] = n1*inv;
		} else {
			nx0[c] = 0.0f;
			nx1[c] = 0.0f;
		}
	}
	hq[0] = fA; hq[1] = fB; hq[2] = fC;
}

// Least squares WITH the quantisation inside (oracle: refit_quantized).  With the selectors fixed the
// error of a channel is a quadratic in its two endpoints, centred at the closed-form solution xu:
// E(e0, e1) - E(xu) = A d0^2 + 2 B d0 d1 + C d1^2 with d = e - xu.  f holds the plain rounding of the
// clamped solution (quantize: p-bits and the centre of the search); every channel then takes, among the
// 3 x 3 pairs of quantised values within one step of that centre, the pair that minimises the form
// (end 0 outer, end 1 inner, -1, 0, +1; first minimum).  A value outside the field's range gets a
// deviation of 1e18: its form value is +inf and never the minimum -- where the least-squares system was solvable.
// In a lane whose system is singular A or C is 0, the sentinel's form value is not +inf and a candidate outside the
// range can win; what such a lane returns is garbage and fit_lane discards it (`live`).
__device__ __forceinline__ void refit_window(const float (&xu0)[4], const float (&xu1)[4], const float (&hq)[3],
	uint32_t cb, uint32_t ab, uint32_t pbk, SubFit& f)
{
	const uint32_t S = pbk ? 1u : 0u;
	const uint32_t P0 = f.pb & 1u, P1 = (f.pb >> 1) & 1u;
	const float fA = hq[0], fC = hq[2], fB2 = hq[1] + hq[1];
	const uint32_t tc = cb ? cb + S : 0u, ta = ab ? ab + S : 0u;
	// The three candidates of every channel as whole words (bc7_packed.h).  q - 1: bit 7 lent to each colour byte
	// (a colour field has at most 7 bits) so that a zero byte borrows from it and not from its neighbour; alpha is the
	// top byte.  Masked to the field width, a candidate outside the range (below 0, above qmax) becomes some code
	// inside it: its deviation is the sentinel and its bytes are never read.
	const uint32_t qmaxw = ((1u << cb) - 1u)*0x010101u | (((1u << ab) - 1u) << 24);
	const uint32_t lo0 = f.q0, lo1 = f.q1;                    // byte c == 0: the channel has no candidate below
	const uint32_t hi0 = f.q0 ^ qmaxw, hi1 = f.q1 ^ qmaxw;    // byte c == 0: none above
	uint32_t dw0[3], dw1[3];
	dw0[0] = dequant_word(code_word(((f.q0 | 0x00808080u) - 0x01010101u) & qmaxw, S, P0), tc, ta);
	dw0[1] = f.e0;
	dw0[2] = dequant_word(code_word((f.q0 + 0x01010101u) & qmaxw, S, P0), tc, ta);
	dw1[0] = dequant_word(code_word(((f.q1 | 0x00808080u) - 0x01010101u) & qmaxw, S, P1), tc, ta);
	dw1[1] = f.e1;
	dw1[2] = dequant_word(code_word((f.q1 + 0x01010101u) & qmaxw, S, P1), tc, ta);
	uint32_t pick = 0;     // byte c: the chosen candidate of end 0 in bits 0..1, of end 1 in bits 4..5
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		const uint32_t bm = 255u << (8*c);
		float dl0[3], dl1[3];
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			dl0[d] = fb(dw0[d], c) - xu0[c];
			dl1[d] = fb(dw1[d], c) - xu1[c];
		}
		dl0[0] = (lo0 & bm) ? dl0[0] : 1.0e18f;
		dl0[2] = (hi0 & bm) ? dl0[2] : 1.0e18f;
		dl1[0] = (lo1 & bm) ? dl1[0] : 1.0e18f;
		dl1[2] = (hi1 & bm) ? dl1[2] : 1.0e18f;
		float best = 3.0e38f;
		uint32_t bi = 0x11u << (8*c);      // the centre unless something is better (the centre is always valid)
#pragma unroll
		for (int i = 0; i < 3; ++i) {
			const float d0 = dl0[i];
			float a0 = fA*d0;
			a0 = a0*d0;
			const float cr = fB2*d0;
#pragma unroll
			for (int j = 0; j < 3; ++j) {
				const float d1 = dl1[j];
				float v = fC*d1;
				v = fmaf(v, d1, a0);
				v = fmaf(cr, d1, v);
				const bool take = v < best;
				best = take ? v : best;
				bi = take ? (uint32_t)(i | (j << 4)) << (8*c) : bi;
			}
		}
		pick |= bi;
	}
	// q + pick - 1 per byte: every chosen candidate lies inside its field's range, so the word sum has no carry or borrow.
	// (A singular lane may choose one outside it: the sum then carries or borrows into the neighbouring bytes, garbage
	// that is discarded with the rest of that lane's result.)
	const uint32_t nq0 = f.q0 + (pick & 0x03030303u) - 0x01010101u;
	const uint32_t nq1 = f.q1 + ((pick >> 4) & 0x03030303u) - 0x01010101u;
	const uint32_t ne0 = dequant_word(code_word(nq0, S, P0), tc, ta);
	const uint32_t ne1 = dequant_word(code_word(nq1, S, P1), tc, ta);
	f.q0 = nq0; f.q1 = nq1; f.e0 = ne0; f.e1 = ne1;
}

// Fit-geometry cache (field-major like the candidate words, one column per thread): what parts A and B of
// fit_lane derive from the texels alone -- axis, mean, the raw projection extremes (before `frac`), the
// extremes of the rotated alpha and the constant pp_sum.  A stream-trip lane writes its fit's words; the
// starts trip, whose four starts of a fit differ only in `frac`, reads them from the lane that fitted the
// same (candidate, fit) in the stream trip.  Word 12 tags the column with that fit (id * 4 + fit index;
// mode 6: fit 0) -- the tag is what says the column still holds it.
#define CF_BC7_GEO_WORDS 13
#define CF_BC7_GEO_NONE 0xFFFFFFFFu
__device__ __forceinline__ uint32_t geo_tag(uint32_t id, uint32_t fi) { return id*4u + (id == 0u ? 0u : fi); }

// What part A's row loop produces, for a fit whose integer statistics are known beforehand: the packed moments of its
// texels in its own (rotated, masked) channel slots (bc7_packed.h) and the extremes lo | hi << 8 of the rotated alpha
// over the block.
struct FitStats {
	uint32_t W[CF_MOM_WORDS];
	uint32_t lohi;
};

// scalar: the fit codes only the rotated alpha channel (modes 4/5 second plane); its start
// endpoints are the exact extremes of that channel (oracle: fit_scalar).
// frac: where the fit starts -- the extremes along the axis pulled in (positive) or pushed out by this
// fraction of their distance (oracle: fitopt.start, cfo_start_frac; 0 = the extremes themselves).
// gmode (wave-uniform): 0 computes parts A and B, 1 computes them and writes them to the lane's own column of
// the geometry cache gbase, 2 reads them from column gsrc instead, 3 (GIVEN instances only) is 1 with the integers of
// part A handed in (gs: the first stream trip, whose fits' moments exist before the fit starts) instead of summed over
// the rows.  NK: palette entries of the selector search
// (assign_lsq_lane).  ITERS: refit rounds of the instance's quality level (one round is straight-line code: it asks
// for no least-squares solution and its `live` is dead).
// owner (unit weights, whose selector search is on the matrix pipe): the fit runs with the whole wave on, and a lane that has no fit walks it on whatever its role
// row holds; `owner` is false there and its result is thrown away by the caller.  The invariant this rests on: inside
// fit_lane and everything it calls, NO store (LDS or global) and NO table or LDS index derived from cb / ab / pbk / ib / mask
// may be reached without `owner` unless it stays in range for any value (weight_row, inv_n, gsrc & 63 do by construction).
// Today the only store is the geometry-cache write below, and it is guarded.
// whole, lohi (unit weights): the fit covers the whole block by its role (mode 6, a plane of modes 4 / 5), and the
// per-block table whose words' upper halves hold the block's raw byte sum, such a fit's search bias (lohi_rawsum; indexed by
// the block alone: in range on any lane).
template <bool UNITW, uint32_t ITERS, int NK = 8, bool GIVEN = false, int CBSZ = 3>
__device__ __forceinline__ void fit_lane(const Tex& tx, uint32_t mask, bool m6, uint32_t khalf,
	uint32_t cb, uint32_t ab, uint32_t pbk, uint32_t ib, const uint32_t (&wt)[4],
	const uint32_t (&yw)[2], bool scalar, float frac, uint32_t* gbase, uint32_t gmode, uint32_t gsrc, const FitStats& gs, bool owner,
	bool whole, const uint32_t* lohi, LaneFit& best)
{
	float axis[4], mean[4];
	float tmin, tmax;
	uint32_t lo, hi, pp_sum, s01, s23;
	if (gmode == 2u) {
		const uint32_t* gc = gbase + gsrc;
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			axis[c] = __uint_as_float(gc[c*CF_WG_THREADS]);
			mean[c] = __uint_as_float(gc[(4 + c)*CF_WG_THREADS]);
		}
		tmin = __uint_as_float(gc[8*CF_WG_THREADS]);
		tmax = __uint_as_float(gc[9*CF_WG_THREADS]);
		const uint32_t lh = gc[10*CF_WG_THREADS];
		lo = lh & 255u; hi = lh >> 8;
		pp_sum = gc[11*CF_WG_THREADS];
		// the subset's channel sums back from the means: mean = s/n to within 2^-22 of s <= 4080, so the
		// product rounds to s exactly
		const float fn = (float)__builtin_popcount(mask);
		s01 = (uint32_t)(mean[0]*fn + 0.5f) | ((uint32_t)(mean[1]*fn + 0.5f) << 16);
		s23 = (uint32_t)(mean[2]*fn + 0.5f) | ((uint32_t)(mean[3]*fn + 0.5f) << 16);
	} else {
		// A: statistics of the subset + extremes of the (rotated) alpha channel
		const uint32_t n = (uint32_t)__builtin_popcount(mask);
		uint32_t s[4] = {0, 0, 0, 0};
		uint32_t q00 = 0, q01 = 0, q02 = 0, q03 = 0, q11 = 0, q12 = 0, q13 = 0, q22 = 0, q23 = 0,
			q33 = 0;
		lo = 255u; hi = 0u;
		if (GIVEN && gmode == 3u) {
			// the same integers as the loop below sums: same floats from here on
			uint32_t q[10];
			mom_unpack(gs.W, s, q);
			q00 = q[0]; q01 = q[1]; q02 = q[2]; q03 = q[3]; q11 = q[4]; q12 = q[5]; q13 = q[6]; q22 = q[7]; q23 = q[8]; q33 = q[9];
			lo = gs.lohi & 255u; hi = UNITW ? lohi_hi(gs.lohi) : gs.lohi >> 8;   // (unit weights: the raw byte sum sits above)
		} else
#pragma unroll 1
		for (uint32_t r = 0; r < 4u; ++r) {
			uint32_t P[4];
			const uint4 pr = *reinterpret_cast<const uint4*>(tx.pl() + 4u*r);
			planes<true>(tx, pr, P);
			const uint32_t a4 = tx.rot == 0u ? pr.w : (tx.rot == 1u ? pr.x : (tx.rot == 2u ? pr.y : pr.z));
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const uint32_t a = (a4 >> (8*j)) & 255u;
				lo = a < lo ? a : lo;
				hi = a > hi ? a : hi;
			}
			const uint32_t m4 = bytemask4((mask >> (4u*r)) & 15u);
			const uint32_t M0 = P[0] & m4, M1 = P[1] & m4, M2 = P[2] & m4, M3 = P[3] & m4;
			s[0] = __builtin_amdgcn_udot4(M0, 0x01010101u, s[0], false);
			s[1] = __builtin_amdgcn_udot4(M1, 0x01010101u, s[1], false);
			s[2] = __builtin_amdgcn_udot4(M2, 0x01010101u, s[2], false);
			s[3] = __builtin_amdgcn_udot4(M3, 0x01010101u, s[3], false);
			q00 = __builtin_amdgcn_udot4(M0, P[0], q00, false);
			q01 = __builtin_amdgcn_udot4(M0, P[1], q01, false);
			q02 = __builtin_amdgcn_udot4(M0, P[2], q02, false);
			q03 = __builtin_amdgcn_udot4(M0, P[3], q03, false);
			q11 = __builtin_amdgcn_udot4(M1, P[1], q11, false);
			q12 = __builtin_amdgcn_udot4(M1, P[2], q12, false);
			q13 = __builtin_amdgcn_udot4(M1, P[3], q13, false);
			q22 = __builtin_amdgcn_udot4(M2, P[2], q22, false);
			q23 = __builtin_amdgcn_udot4(M2, P[3], q23, false);
			q33 = __builtin_amdgcn_udot4(M3, P[3], q33, false);
		}
		// n q_cd - s_c s_d on exact floats, one fused multiply-add per term (bc7_packed.h: cov_term); n, q and s converted once each
		const float fn = (float)n, f0 = (float)s[0], f1 = (float)s[1], f2 = (float)s[2], f3 = (float)s[3];
		const float C00 = cov_term(fn, q00, f0, f0), C01 = cov_term(fn, q01, f0, f1);
		const float C02 = cov_term(fn, q02, f0, f2), C03 = cov_term(fn, q03, f0, f3);
		const float C11 = cov_term(fn, q11, f1, f1), C12 = cov_term(fn, q12, f1, f2);
		const float C13 = cov_term(fn, q13, f1, f3), C22 = cov_term(fn, q22, f2, f2);
		const float C23 = cov_term(fn, q23, f2, f3), C33 = cov_term(fn, q33, f3, f3);

		float bestd = C00;
		float v0 = C00, v1 = C01, v2 = C02, v3 = C03;
		if (C11 > bestd) { bestd = C11; v0 = C01; v1 = C11; v2 = C12; v3 = C13; }
		if (C22 > bestd) { bestd = C22; v0 = C02; v1 = C12; v2 = C22; v3 = C23; }
		if (C33 > bestd) { bestd = C33; v0 = C03; v1 = C13; v2 = C23; v3 = C33; }
#pragma unroll
		for (int it = 0; it < 3; ++it) {
			float r0 = C00*v0; r0 = fmaf(C01, v1, r0); r0 = fmaf(C02, v2, r0); r0 = fmaf(C03, v3, r0);
			float r1 = C01*v0; r1 = fmaf(C11, v1, r1); r1 = fmaf(C12, v2, r1); r1 = fmaf(C13, v3, r1);
			float r2 = C02*v0; r2 = fmaf(C12, v1, r2); r2 = fmaf(C22, v2, r2); r2 = fmaf(C23, v3, r2);
			float r3 = C03*v0; r3 = fmaf(C13, v1, r3); r3 = fmaf(C23, v2, r3); r3 = fmaf(C33, v3, r3);
			v0 = r0; v1 = r1; v2 = r2; v3 = r3;
		}
		const float mx = fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3)));
#pragma unroll
		for (int c = 0; c < 4; ++c) axis[c] = 0.0f;
		if (mx > 0.0f) {
			const float im = cf_rcp_tested(mx);
			v0 = v0*im; v1 = v1*im; v2 = v2*im; v3 = v3*im;
			float l2 = v0*v0;
			l2 = fmaf(v1, v1, l2);
			l2 = fmaf(v2, v2, l2);
			l2 = fmaf(v3, v3, l2);
			const float is = cf_rcp_ranged(sqrtf(l2));
			axis[0] = v0*is; axis[1] = v1*is; axis[2] = v2*is; axis[3] = v3*is;
		}

		// B: extremes of the projection on the axis
		const float in = inv_n(n);
#pragma unroll
		for (int c = 0; c < 4; ++c)
			mean[c] = (float)s[c]*in;
		tmin = 3.0e38f; tmax = -3.0e38f;
#pragma unroll 1
		for (uint32_t r = 0; r < 4u; ++r) {
			const uint4 rw = *reinterpret_cast<const uint4*>(tx.tp() + 4u*r);
			const uint32_t raw[4] = {rw.x, rw.y, rw.z, rw.w};
			const uint32_t mrow = (mask >> (4u*r)) & 15u;
			if constexpr (UNITW) {
				// one select per texel, then two texels per v_min3_f32 / v_max3_f32 (bc7_packed.h: proj_extremes2)
				float tm[4];
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const uint32_t p = texel<true>(tx, raw[j]);
					float t = axis[0]*(fb(p, 0) - mean[0]);
					t = fmaf(axis[1], fb(p, 1) - mean[1], t);
					t = fmaf(axis[2], fb(p, 2) - mean[2], t);
					t = fmaf(axis[3], fb(p, 3) - mean[3], t);
					tm[j] = proj_or_nan(t, (mrow >> j) & 1u);
				}
				proj_extremes2(tmin, tmax, tm[0], tm[1]);
				proj_extremes2(tmin, tmax, tm[2], tm[3]);
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const uint32_t p = texel<true>(tx, raw[j]);
					const bool m = (mrow >> j) & 1u;
					float t = axis[0]*(fb(p, 0) - mean[0]);
					t = fmaf(axis[1], fb(p, 1) - mean[1], t);
					t = fmaf(axis[2], fb(p, 2) - mean[2], t);
					t = fmaf(axis[3], fb(p, 3) - mean[3], t);
					tmin = m ? fminf(tmin, t) : tmin;
					tmax = m ? fmaxf(tmax, t) : tmax;
				}
			}
		}
		// sum over the subset of sum_c p_c^2 (channels that are not coded have p = 0), or of the
		// weighted squares on the perceptual axes
		pp_sum = UNITW ? q00 + q11 + q22 + q33 : ycc_pp_sum(tx, mask, yw);
		if constexpr (UNITW) {
			// the selector search runs without its C operand: the sum of the subset's raw bytes, times 256, leaves the
			// constant here (bc7_packed.h).  By the lane's role: a whole-block fit's channel set hides raw channels from s.
			const uint32_t bias = whole ? lohi_rawsum((GIVEN && gmode == 3u) ? gs.lohi : lohi[tx.boff >> 2])
				: search_bias_part(s[0], s[1], s[2], s[3], n, !(tx.chmask & 8u));
			pp_sum = search_pp_fold(pp_sum, bias);
		}
		s01 = s[0] | (s[1] << 16);
		s23 = s[2] | (s[3] << 16);
		if ((GIVEN ? gmode != 0u : gmode == 1u) && (UNITW ? owner : true)) {   // 1 or 3; owner: see the call (a lane without a fit stores nothing)
			uint32_t lane;
			CF_FRESH_LANE(lane);
			uint32_t* gc = gbase + lane;
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				gc[c*CF_WG_THREADS] = __float_as_uint(axis[c]);
				gc[(4 + c)*CF_WG_THREADS] = __float_as_uint(mean[c]);
			}
			gc[8*CF_WG_THREADS] = __float_as_uint(tmin);
			gc[9*CF_WG_THREADS] = __float_as_uint(tmax);
			gc[10*CF_WG_THREADS] = lo | (hi << 8);
			gc[11*CF_WG_THREADS] = pp_sum;
		}
	}
	{
		const float d = (tmax - tmin)*frac;
		tmin = tmin + d;
		tmax = tmax - d;
	}
	float x0[4], x1[4];
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		x0[c] = clamp255(fmaf(axis[c], tmin, mean[c]));
		x1[c] = clamp255(fmaf(axis[c], tmax, mean[c]));
	}
	if (scalar) {
		const float flo = (float)lo, fhi = (float)hi;
		const float d = (fhi - flo)*frac;
		x0[0] = 0.0f; x0[1] = 0.0f; x0[2] = 0.0f; x0[3] = clamp255(flo + d);
		x1[0] = 0.0f; x1[1] = 0.0f; x1[2] = 0.0f; x1[3] = clamp255(fhi - d);
	}
	// C/D then E rounds.  A round that does not improve ends the lane's search (the same
	// input would give the same output again): x0/x1 always hold the refit of the newest
	// selectors and `live` says whether they belong to the best fit so far.
	// The fit's four small parameters travel through the rounds as ONE word (cb | ab << 4 | pbk << 8 |
	// ib << 12), unpacked where a step needs them from a copy the compiler cannot see through -- as four
	// registers held across the selector search they were what pushed the 128-register build into scratch.
	uint32_t geo = cb | (ab << 4) | (pbk << 8) | (ib << 12);
	asm volatile("" : "+v"(geo));
#define G_CB (geo & 15u)
#define G_AB ((geo >> 4) & 15u)
#define G_PBK ((geo >> 8) & 15u)
#define G_IB (geo >> 12)
	SubFit q;
	quantize<UNITW>(x0, x1, G_CB, G_AB, G_PBK, wt, q);
	best.q0 = q.q0; best.q1 = q.q1; best.pb = q.pb;
	bool live;
	float hq[3];
	// (matrix pipe: the whole wave is on here, so the A operand is loaded where it is used)
	uint32_t arow[4];
	arow_load<UNITW>(tx.tile_, tx.boff, arow);
	assign_lsq_lane<UNITW, NK, CBSZ>(tx, mask, m6, khalf, G_IB, yw, pp_sum, ITERS > 0u, q.e0, q.e1, arow, best, x0, x1, hq, live, s01, s23);
	// (Highest's two rounds stay a loop: unrolled, the second copy of the search spills 12 vector registers)
#pragma unroll 1
	for (uint32_t r = 0; r < ITERS; ++r) {
		LaneFit cur;
		bool ok;
		asm volatile("" : "+v"(geo));
		{
			// x0 / x1: the unclamped least-squares solution; rounded from its clamped copy, then searched
			float c0[4], c1[4];
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				c0[c] = clamp255(x0[c]);
				c1[c] = clamp255(x1[c]);
			}
			quantize<UNITW>(c0, c1, G_CB, G_AB, G_PBK, wt, q);
		}
		if (!(CF_BC7_ABLATE & 8)) refit_window(x0, x1, hq, G_CB, G_AB, G_PBK, q);
		cur.q0 = q.q0; cur.q1 = q.q1; cur.pb = q.pb;
		arow_load<UNITW>(tx.tile_, tx.boff, arow);
		assign_lsq_lane<UNITW, NK, CBSZ>(tx, mask, m6, khalf, G_IB, yw, pp_sum, r + 1u < ITERS, q.e0, q.e1, arow, cur, x0, x1, hq, ok, s01, s23);
		const bool better = live && cur.err < best.err;
		if (better)
			best = cur;
		live = better && ok;
	}
#undef G_CB
#undef G_AB
#undef G_PBK
#undef G_IB
}

__device__ __forceinline__ uint32_t w2i(uint32_t w, uint32_t ib)
{
	return (w*((1u << ib) - 1u) + 32u) >> 6;
}

// Bit-pack the winning candidate(s) with the whole wavefront (same layout as the oracle's
// pack()).  One block per wave (pair = false, 64 lanes) or two (pair = true, 32 lanes each):
// every lane reads its block's winner from that lane's LDS column, forms its bit fields
// (value, offset) and the 128-bit block is the OR of the contributions of the group.
// Field slots f (a lane owns slot hl, and hl + 32 too when its group has only 32 lanes):
//    0..15 : first index field, texel = f        16..31 : second index field, texel = f - 16
//   32..55 : endpoint field (channel-major)      56..61 : p-bits      62 : mode/partition/... header
// What a slot holds, where it stands and where its value comes from is one word of the shape's row of k_bc7_pack
// (bc7_pack.h); what depends on the partition -- the anchors, the endpoint orders, the header's value -- is formed here.
__device__ __forceinline__ uint4 pack_block_group(const uint32_t* wcol, uint32_t id, uint32_t lane,
	bool pair)
{
	const uint32_t h = lane >> 5, hl = pair ? (lane & 31u) : lane, hbase = pair ? (lane & 32u) : 0u;
	// the shape's row: its candidate word, then one word per field slot (bc7_pack.h)
	// (the winner's id is below 384; the clamp keeps the row inside the table whatever a lane without a block holds)
	const uint32_t shape = cf_bc7_cand_index(id);
	const uint32_t* row = k_bc7_pack.w + (shape < CF_CAND_TABLE_N ? shape : CF_CAND_TABLE_N - 1u)*CF_PACK_ROW;
	const uint32_t cw = row[0];
	const uint32_t mode = CF_CAND_MODE(cw), ns = CF_CAND_NS(cw);
	const uint32_t part = ns > 1u ? id & 63u : 0u;
	const uint32_t ibc = CF_CAND_IB(cw), iba = CF_CAND_IB2(cw);
	const uint32_t p2 = k_part2[part], p3 = k_part3[part];
	uint32_t a1 = 0, a2 = 0;
	if (ns == 2u) a1 = k_anchor2[part];
	else if (ns == 3u) { a1 = k_anchor3a[part]; a2 = k_anchor3b[part]; }

	// texel t = hl & 15: subset, both indices
	const uint32_t t = hl & 15u;
	const uint32_t sb = ns == 1u ? 0u : (ns == 2u ? ((p2 >> t) & 1u) : ((p3 >> (2u*t)) & 3u));
	const uint32_t wv = (wcol[(7u + (t >> 2))*CF_WG_THREADS] >> (8u*(t & 3u))) & 255u;
	const uint32_t ws = (wcol[(11u + (t >> 2))*CF_WG_THREADS] >> (8u*(t & 3u))) & 255u;
	uint32_t idxv = w2i(wv, ibc);
	uint32_t idxs = iba ? w2i(ws, iba) : 0u;
	// anchors decide the endpoint order of their subset (texel a lives in lane hbase + a)
	const uint32_t i0 = (uint32_t)cf_bperm((int)idxv, (uint32_t)((int)hbase));
	const uint32_t i1 = (uint32_t)cf_bperm((int)idxv, (uint32_t)((int)(hbase + a1)));
	const uint32_t i2 = (uint32_t)cf_bperm((int)idxv, (uint32_t)((int)(hbase + a2)));
	const uint32_t is0 = (uint32_t)cf_bperm((int)idxs, (uint32_t)((int)hbase));
	const uint32_t sw0 = i0 >> (ibc - 1u);
	const uint32_t sw1 = ns > 1u ? i1 >> (ibc - 1u) : 0u;
	const uint32_t sw2 = ns > 2u ? i2 >> (ibc - 1u) : 0u;
	const uint32_t sws = iba ? is0 >> (iba - 1u) : 0u;
	const uint32_t swmask = sw0 | (sw1 << 1) | (sw2 << 2);
	idxv = ((swmask >> sb) & 1u) ? ((1u << ibc) - 1u) - idxv : idxv;
	idxs = sws ? ((1u << iba) - 1u) - idxs : idxs;
	const uint32_t swall = swmask | (sws << 3);      // endpoint orders: subsets 0..2, the scalar plane
	// the first index field loses the bit of every anchor before the texel
	const uint32_t before = (t > 0u ? 1u : 0u) + ((ns >= 2u && t > a1) ? 1u : 0u) + ((ns == 3u && t > a2) ? 1u : 0u);
	const uint32_t pbn = cf_bc7_pack_pbn(mode);
	uint32_t hval = (1u << mode) | (part << (mode + 1u));
	if (CF_CAND_P45(cw))
		hval = (1u << mode) | (CF_CAND_ROT(cw) << (mode + 1u + pbn)) | (CF_CAND_ISEL(cw) << (mode + 1u + pbn + 2u));

	uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
	const uint32_t npass = pair ? 2u : 1u;
	for (uint32_t pass = 0; pass < npass; ++pass) {
		const uint32_t f = hl + 32u*pass;
		const uint32_t s = row[1u + f];
		const uint32_t kind = CF_PACK_KIND(s);
		const uint32_t sbit = (swall >> CF_PACK_ORDER(s)) & 1u;
		const uint32_t cword = wcol[(CF_PACK_WORD(s) ^ (CF_PACK_FLIPW(s) & sbit))*CF_WG_THREADS];
		const uint32_t cval = (cword >> (CF_PACK_SHIFT(s) ^ (CF_PACK_FLIPS(s) & sbit))) & (CF_PACK_BYTE(s) ? 255u : 1u);
		uint32_t val = kind == CF_PACK_KIND_COL ? cval : (kind == CF_PACK_KIND_HDR ? hval : (kind == CF_PACK_KIND_IDX1 ? idxv : idxs));
		val = CF_PACK_HAVE(s) ? val : 0u;
		const uint32_t off = CF_PACK_OFF(s) - (f < 16u ? before : 0u);
		const uint32_t wi = off >> 5, sh = off & 31u;
		const unsigned long long vv = (unsigned long long)val << sh;
		const uint32_t lo = (uint32_t)vv, hi = (uint32_t)(vv >> 32);
		w0 |= wi == 0u ? lo : 0u;
		w1 |= wi == 1u ? lo : (wi == 0u ? hi : 0u);
		w2 |= wi == 2u ? lo : (wi == 1u ? hi : 0u);
		w3 |= wi == 3u ? lo : (wi == 2u ? hi : 0u);
	}
	uint4 r;
	r.x = cf_group_or_u32(w0, pair, h);
	r.y = cf_group_or_u32(w1, pair, h);
	r.z = cf_group_or_u32(w2, pair, h);
	r.w = cf_group_or_u32(w3, pair, h);
	return r;
}

// The 14 integer moments of a set of texels: channel sums and sums of products.  Exact unsigned integers, so the
// moments of a subset are the block's minus those of the other subsets, bit for bit.
struct Moments {
	uint32_t s[4];
	uint32_t q00, q01, q02, q03, q11, q12, q13, q22, q23, q33;
};

// Per-block table of the whole block's moments (built once per workgroup, kernel prologue), 10 words per block:
// words 0..3 = q_cc | s_c << 20 (q <= 16 * 255^2 < 2^20, s <= 16 * 255 < 2^12), words 4..9 = q01 q02 q03 q12 q13 q23.
// The block's own channel set is applied: every alpha term of an opaque block is zero, as planes() zeroes its plane.
#define CF_BC7_MOM_WORDS 10
__device__ __forceinline__ void block_moments_put(const uint32_t* plan, uint32_t* mom, uint32_t t)
{
	const uint32_t b = t >> 4, m = t & 15u;
	if (m >= CF_BC7_MOM_WORDS)
		return;
	// channel pair (ca, cb) of word m
	const uint32_t ca = m < 4u ? m : (m < 7u ? 0u : (m < 9u ? 1u : 2u));
	const uint32_t cb = m < 4u ? m : (m < 7u ? m - 3u : (m < 9u ? m - 5u : 3u));
	const uint32_t* pb = plan + b*16u;
	const bool opaque = (pb[3] & pb[7] & pb[11] & pb[15]) == 0xFFFFFFFFu;
	uint32_t q = 0, sm = 0;
#pragma unroll
	for (uint32_t r = 0; r < 4u; ++r) {
		const uint32_t A = (opaque && ca == 3u) ? 0u : pb[4u*r + ca], B = (opaque && cb == 3u) ? 0u : pb[4u*r + cb];
		q = __builtin_amdgcn_udot4(A, B, q, false);
		sm = __builtin_amdgcn_udot4(A, 0x01010101u, sm, false);
	}
	mom[b*CF_BC7_MOM_WORDS + m] = m < 4u ? q | (sm << 20) : q;
}

// Moments of one (TWO = false) or two disjoint texel sets of a block in one pass over its planar rows.
// A4 = false: the block is opaque, every term that carries the fourth channel is an exact zero and is left out.
template <bool A4, bool TWO>
__device__ __forceinline__ void moments_rows(const Tex& tx, uint32_t mask1, uint32_t mask2, Moments& a, Moments& b)
{
#pragma unroll
	for (int c = 0; c < 4; ++c) { a.s[c] = 0; b.s[c] = 0; }
	a.q00 = a.q01 = a.q02 = a.q03 = a.q11 = a.q12 = a.q13 = a.q22 = a.q23 = a.q33 = 0;
	b.q00 = b.q01 = b.q02 = b.q03 = b.q11 = b.q12 = b.q13 = b.q22 = b.q23 = b.q33 = 0;
#pragma unroll 1
	for (uint32_t r = 0; r < 4u; ++r) {
		uint32_t P[4];
		planes<false>(tx, *reinterpret_cast<const uint4*>(tx.pl() + 4u*r), P);
#pragma unroll
		for (int k = 0; k < (TWO ? 2 : 1); ++k) {
			Moments& o = k ? b : a;
			const uint32_t m4 = bytemask4(((k ? mask2 : mask1) >> (4u*r)) & 15u);
			const uint32_t M0 = P[0] & m4, M1 = P[1] & m4, M2 = P[2] & m4, M3 = A4 ? P[3] & m4 : 0u;
			o.s[0] = __builtin_amdgcn_udot4(M0, 0x01010101u, o.s[0], false);
			o.s[1] = __builtin_amdgcn_udot4(M1, 0x01010101u, o.s[1], false);
			o.s[2] = __builtin_amdgcn_udot4(M2, 0x01010101u, o.s[2], false);
			if (A4) o.s[3] = __builtin_amdgcn_udot4(M3, 0x01010101u, o.s[3], false);
			o.q00 = __builtin_amdgcn_udot4(M0, P[0], o.q00, false);
			o.q01 = __builtin_amdgcn_udot4(M0, P[1], o.q01, false);
			o.q02 = __builtin_amdgcn_udot4(M0, P[2], o.q02, false);
			if (A4) o.q03 = __builtin_amdgcn_udot4(M0, P[3], o.q03, false);
			o.q11 = __builtin_amdgcn_udot4(M1, P[1], o.q11, false);
			o.q12 = __builtin_amdgcn_udot4(M1, P[2], o.q12, false);
			if (A4) o.q13 = __builtin_amdgcn_udot4(M1, P[3], o.q13, false);
			o.q22 = __builtin_amdgcn_udot4(M2, P[2], o.q22, false);
			if (A4) o.q23 = __builtin_amdgcn_udot4(M2, P[3], o.q23, false);
			if (A4) o.q33 = __builtin_amdgcn_udot4(M3, P[3], o.q33, false);
		}
	}
}

// The block's moments (table words tw) minus those of a (TWO: and of b): the subset that was not summed
template <bool A4, bool TWO>
__device__ __forceinline__ Moments moments_rest(const uint32_t* tw, const Moments& a, const Moments& b)
{
	Moments o;
	const uint32_t w0 = tw[0], w1 = tw[1], w2 = tw[2], w3 = A4 ? tw[3] : 0u;
#define CF_REST(f, tot) o.f = (tot) - a.f - (TWO ? b.f : 0u)
	CF_REST(s[0], w0 >> 20); CF_REST(s[1], w1 >> 20); CF_REST(s[2], w2 >> 20);
	CF_REST(q00, w0 & 0xFFFFFu); CF_REST(q11, w1 & 0xFFFFFu); CF_REST(q22, w2 & 0xFFFFFu);
	CF_REST(q01, tw[4]); CF_REST(q02, tw[5]); CF_REST(q12, tw[7]);
	if (A4) {
		CF_REST(s[3], w3 >> 20); CF_REST(q33, w3 & 0xFFFFFu);
		CF_REST(q03, tw[6]); CF_REST(q13, tw[8]); CF_REST(q23, tw[9]);
	} else {
		o.s[3] = 0; o.q33 = 0; o.q03 = 0; o.q13 = 0; o.q23 = 0;
	}
#undef CF_REST
	return o;
}

// Partition score of the two-phase search (oracle: subset_residual): the scatter of the
// subset that no line through its mean can capture, (trace(C) - a'Ca)/n, with a = the
// power-iterated principal axis.  Same statistics and axis arithmetic as fit_lane; mo: the subset's moments.
// A4 = false: the block is opaque (the alpha plane is masked to zero), so every term that
// carries the fourth channel is an exact zero and is left out -- same result, bit for bit.
template <bool A4>
__device__ __forceinline__ float subset_residual(const Moments& mo, uint32_t mask, float& along)
{
	const uint32_t n = (uint32_t)__builtin_popcount(mask);
	const uint32_t s[4] = {mo.s[0], mo.s[1], mo.s[2], mo.s[3]};
	const uint32_t q00 = mo.q00, q01 = mo.q01, q02 = mo.q02, q03 = mo.q03, q11 = mo.q11, q12 = mo.q12, q13 = mo.q13,
		q22 = mo.q22, q23 = mo.q23, q33 = mo.q33;
	// (the covariance terms as in fit_lane: cov_term on exact floats; an opaque block's fourth-channel terms are +0 and unused)
	const float fn = (float)n, f0 = (float)s[0], f1 = (float)s[1], f2 = (float)s[2], f3 = (float)s[3];
	const float C00 = cov_term(fn, q00, f0, f0), C01 = cov_term(fn, q01, f0, f1);
	const float C02 = cov_term(fn, q02, f0, f2), C03 = cov_term(fn, q03, f0, f3);
	const float C11 = cov_term(fn, q11, f1, f1), C12 = cov_term(fn, q12, f1, f2);
	const float C13 = cov_term(fn, q13, f1, f3), C22 = cov_term(fn, q22, f2, f2);
	const float C23 = cov_term(fn, q23, f2, f3), C33 = cov_term(fn, q33, f3, f3);
	float bestd = C00;
	float v0 = C00, v1 = C01, v2 = C02, v3 = C03;
	if (C11 > bestd) { bestd = C11; v0 = C01; v1 = C11; v2 = C12; v3 = C13; }
	if (C22 > bestd) { bestd = C22; v0 = C02; v1 = C12; v2 = C22; v3 = C23; }
	if (A4 && C33 > bestd) { bestd = C33; v0 = C03; v1 = C13; v2 = C23; v3 = C33; }
	// C * v; the fourth row and column are exact zeros for an opaque block
#define CF_MATVEC(o0, o1, o2, o3) \
	float o0 = C00*v0; o0 = fmaf(C01, v1, o0); o0 = fmaf(C02, v2, o0); if (A4) o0 = fmaf(C03, v3, o0); \
	float o1 = C01*v0; o1 = fmaf(C11, v1, o1); o1 = fmaf(C12, v2, o1); if (A4) o1 = fmaf(C13, v3, o1); \
	float o2 = C02*v0; o2 = fmaf(C12, v1, o2); o2 = fmaf(C22, v2, o2); if (A4) o2 = fmaf(C23, v3, o2); \
	float o3 = 0.0f; \
	if (A4) { o3 = C03*v0; o3 = fmaf(C13, v1, o3); o3 = fmaf(C23, v2, o3); o3 = fmaf(C33, v3, o3); }
#pragma unroll
	for (int it = 0; it < 3; ++it) {
		CF_MATVEC(r0, r1, r2, r3)
		v0 = r0; v1 = r1; v2 = r2; v3 = r3;
	}
	float mx = fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fabsf(v2));
	if (A4) mx = fmaxf(mx, fabsf(v3));
	float tr = C00 + C11;
	tr = tr + C22;
	if (A4) tr = tr + C33;
	float res = 0.0f;
	along = 0.0f;
	if (mx > 0.0f) {
		const float im = cf_rcp_tested(mx);
		v0 = v0*im; v1 = v1*im; v2 = v2*im; v3 = A4 ? v3*im : 0.0f;
		CF_MATVEC(w0, w1, w2, w3)
		float num = v0*w0;
		num = fmaf(v1, w1, num);
		num = fmaf(v2, w2, num);
		if (A4) num = fmaf(v3, w3, num);
		float den = v0*v0;
		den = fmaf(v1, v1, den);
		den = fmaf(v2, v2, den);
		if (A4) den = fmaf(v3, v3, den);
		const float lam = num*cf_rcp_ranged(den);
		const float in = inv_n(n);
		res = (tr - lam)*in;
		res = res > 0.0f ? res : 0.0f;
		const float al = lam*in;
		along = al > 0.0f ? al : 0.0f;
	}
#undef CF_MATVEC
	return res;
}

// The (error, id) key of a candidate, ordered like the pair.  Unit weights: a block's error is at most
// 16 * 4 * 255^2 < 2^22 and ids are below 384 < 2^9, so error << 9 | id is one word and its group minimum a 32-bit
// DPP reduction; a column that holds no candidate (error 0xFFFFFFFF) gets 0xFFFFFFFE, below `taken` and above every
// candidate.  The perceptual metric's weighted errors do not fit: 64 bits.
template <bool UNITW> struct CandKey;
template <> struct CandKey<true> {
	typedef uint32_t T;
	static __device__ __forceinline__ T make(uint32_t err, uint32_t id) { return err == 0xFFFFFFFFu ? 0xFFFFFFFEu : (err << 9) | id; }
	static __device__ __forceinline__ T group_min(T k, bool pair, uint32_t h) { return cf_group_min_u32(k, pair, h); }
};
template <> struct CandKey<false> {
	typedef unsigned long long T;
	static __device__ __forceinline__ T make(uint32_t err, uint32_t id) { return ((unsigned long long)err << 32) | id; }
	static __device__ __forceinline__ T group_min(T k, bool pair, uint32_t h) { return cf_group_min_u64(k, pair, h); }
};

// Geometry of fit kf of candidate id (oracle: fit_geometry): mode, partition / rotation / index selector,
// the channels and precisions the fit codes, its index width and its texels.
struct FitGeo {
	uint32_t mode, part, rot, isel, ns, nfits, cb, ab, pbk, ib, mask, chm;
	bool m6, planes45, sca;
};

// It is read from what the candidate's leader stored with it: the candidate word (word 6 of its column,
// bc7_cand.h) by bit-field extracts, the fit's texels by one table load.  The word of a column that holds no candidate is
// whatever the word held before: every field is masked to its range, and the lanes that read it are idle.
__device__ __forceinline__ FitGeo cand_geo(uint32_t cw, uint32_t id, uint32_t kf)
{
	const cf_bc7_cand_fit c = cf_bc7_cand_fit_of(cw, id, kf);
	FitGeo g;
	g.mode = c.mode; g.part = c.part; g.rot = c.rot; g.isel = c.isel; g.ns = c.ns; g.nfits = c.nfits;
	g.cb = c.cb; g.ab = c.ab; g.pbk = c.pbk; g.ib = c.ib; g.chm = c.chm;
	g.m6 = c.m6; g.planes45 = c.planes45; g.sca = c.sca;
	g.mask = k_bc7_masks.m[c.mi];
	return g;
}

// Geometry of fit kf of the candidate stored in column wc
__device__ __forceinline__ FitGeo column_geo(const uint32_t* wc, uint32_t id, uint32_t kf)
{
	return cand_geo(wc[6*CF_WG_THREADS], id, kf);
}

// The geometry-cache tag of a candidate whose geometry is at hand (geo_tag(id, fi) without the compare on id)
__device__ __forceinline__ uint32_t geo_tag(const FitGeo& g, uint32_t id, uint32_t fi) { return id*4u + (g.m6 ? 0u : fi); }
// Lane that ran fit fi of the candidate whose leader (first-fit lane) is wl, in the stream trips' layouts
// (a guess checked by the tag: a wrong one only costs the fall-back to the full fit).
__device__ __forceinline__ uint32_t geo_src(const FitGeo& g, uint32_t fi, uint32_t wl, bool lay32)
{
	uint32_t s = wl + fi;                                          // partitions: the subsets in consecutive lanes
	if (g.m6) s = wl;                                              // mode 6: both palette halves fit the same geometry
	else if (g.planes45) s = fi ? wl + (lay32 ? (g.mode == 5u ? 4u : 1u) : 12u) : wl;   // modes 5 / 4: scalar plane s2off lanes up
	else if (lay32 && g.ns == 3u && fi == 2u)                      // 32-lane second pass: subset 2 of slot s in lane s
		s = (wl & 32u) + (((wl & 31u) - 11u) >> 1);
	return s & 63u;
}

// and / or on a word of LDS with no value returned (ds_and_b32 / ds_or_b32): the lanes of a wave that meet in one word
// are applied one after the other by the LDS itself.
__device__ __forceinline__ void cf_lds_and(uint32_t* p, uint32_t v)
{
	(void)__hip_atomic_fetch_and(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void cf_lds_or(uint32_t* p, uint32_t v)
{
	(void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Store a fit (quantised fields, weights, error) into fit slot kf of a candidate's column; its p-bits go by
// column_put_pbits.  The fields a fit owns alone are plain stores.  The four weight words are shared with the
// candidate's other fits, which may store in the same instruction: there a fit clears and sets the bytes of its own
// texels by and / or (bc7_packed.h: cf_put_weights), which needs no order between the fits.
__device__ __forceinline__ void column_put_fit(uint32_t* wc, const FitGeo& g, uint32_t kf, uint32_t q0, uint32_t q1,
	const uint32_t (&w)[4], uint32_t err)
{
	const uint32_t fq0 = g.planes45 ? (g.sca ? 4u : 0u) : 2u*kf;
	wc[fq0*CF_WG_THREADS] = q0;
	wc[(fq0 + 1u)*CF_WG_THREADS] = q1;
	wc[(15u + kf)*CF_WG_THREADS] = err;
#pragma unroll
	for (uint32_t rr = 0; rr < 4u; ++rr) {
		if (g.sca)
			wc[(11u + rr)*CF_WG_THREADS] = w[rr];
		else {
			const cf_put_masks wm = cf_put_weights(g.mask, rr, w[rr]);
			cf_lds_and(&wc[(7u + rr)*CF_WG_THREADS], wm.keep);
			cf_lds_or(&wc[(7u + rr)*CF_WG_THREADS], wm.set);
		}
	}
}

// The p-bits of fit kf into the p-bit word of the column (word 6, below the candidate's fields): a read-modify-write,
// so the fits of a candidate take it one at a time (the callers' loops).
__device__ __forceinline__ void column_put_pbits(uint32_t* wc, uint32_t kf, uint32_t pb)
{
	const uint32_t pw = wc[6*CF_WG_THREADS];
	wc[6*CF_WG_THREADS] = (pw & ~(3u << (2u*kf))) | (pb << (2u*kf));
}


// Rows of k_bc7_roles for the two halves of a wave in the 32-lane layouts, half 1's in bits 8..10 (wave-uniform).
// abal: ballot of the texels with alpha, 16 per half; gb: bit 0 / 32 = half 0 / 1 walks the second pass (one block per
// wave: bit 0, and the upper lanes have no roles).
__device__ __forceinline__ uint32_t role_rows32(uint32_t st, unsigned long long abal, unsigned long long gb, bool pair)
{
	const uint32_t a0 = ((uint32_t)abal & 0xFFFFu) != 0u ? 1u : 0u, a1 = ((uint32_t)(abal >> 32) & 0xFFFFu) != 0u ? 1u : 0u;
	const uint32_t g0 = (uint32_t)gb & 1u, g1 = (uint32_t)(gb >> 32) & 1u;
	const uint32_t r0 = st == 0u ? a0 : (g0 ? 2u + a0 : CF_ROLE_ROW_NONE);
	const uint32_t r1 = !pair ? CF_ROLE_ROW_NONE : (st == 0u ? a1 : (g1 ? 2u + a1 : CF_ROLE_ROW_NONE));
	return r0 | (r1 << 8);
}

// Encode one block with the whole wavefront.  tp: the block's 16 texels in LDS
// (colour mask already applied), identical for every lane.
// LEVEL: the quality level (0 Lowest .. 4 Highest).  Its whole search budget -- refit rounds, list length,
// perturbation rounds, move sets, streams, the lane layout -- is a compile-time constant of the instance: held as
// run-time scalars across every phase the budget cost 53 spilled SGPRs in the Normal build, and every lane-role
// expression selected its layout again.
template <bool UNITW, bool WIDE, int LEVEL>
__device__ __forceinline__ uint4 encode_blocks(const uint32_t* tile, const uint32_t* plan, const uint32_t* yccp, const uint32_t* mom, const uint32_t* lohi, uint32_t b,
	bool pair, uint32_t* cbase, uint32_t* gbase, const cf_kparams& kp)
{
	uint32_t lane;
	CF_FRESH_LANE(lane);
#define L_CSLOT (cbase + lane)
	// lane whose column holds the k-th best candidate of this lane's group (list words 20 / 21 of the lane's column)
#define TOP_LANE(k) ((L_CSLOT[(20u + ((k) >> 2))*CF_WG_THREADS] >> (8u*((k) & 3u))) & 255u)
	// pair: blocks b and b + 1 at Low or Normal, one per half wavefront
#define L_H (lane >> 5)
#define L_HBASE (pair ? (lane & 32u) : 0u)
	// (the block's LDS pointers are expressions of the current lane id too: half h of a pair)
#define B_TP (tile + (pair ? b + L_H : b)*16u)
#define B_OFF ((pair ? b + L_H : b)*16u)
	// perceptual axis weights as 16-bit pairs (wY | wCr << 16, wCb | wA << 16); kp.flags holds the bytes
	const uint32_t ywrg = (kp.flags & 255u) | (((kp.flags >> 8) & 255u) << 16);
	const uint32_t ywba = ((kp.flags >> 16) & 255u) | (((kp.flags >> 24) & 127u) << 16);
	// lanes 0..15 of each group test their block's alpha
	const unsigned long long abal = __ballot((lane & 31u) < 16u && (B_TP[lane & 15u] >> 24) != 255u);
	const bool has_alpha = pair ? ((uint32_t)(L_H ? abal >> 32 : abal) & 0xFFFFu) != 0u
		: ((uint32_t)abal & 0xFFFFu) != 0u;
	const bool any_alpha = pair ? abal != 0ull : has_alpha;
	// inside the stream loop the flag is an expression of the CURRENT lane id (a loop-invariant per-lane value, and
	// everything derived from it, would be hoisted out of the loop and held in registers through every trip)
#define H_ALPHA (pair ? ((uint32_t)(L_H ? abal >> 32 : abal) & 0xFFFFu) != 0u : ((uint32_t)abal & 0xFFFFu) != 0u)
	// Low runs Normal's candidate set without the refit round (oracle: quality_budget): `quality`
	// below selects the LAYOUT, so Low is mapped onto Normal's
	static_assert(LEVEL >= 0 && LEVEL <= 4 && WIDE == (LEVEL >= 3), "levels 0..2 use the 32-lane layouts, 3 and 4 the wide one");
	constexpr uint32_t iters = LEVEL >= 4 ? 2u : (LEVEL >= 2 ? 1u : 0u);   // refit rounds 0,0,1,1,2
	// WIDE (Highest): the 64-lane layout with both streams.  Otherwise the 32-lane layouts: Low and
	// High walk Normal's candidate set (High adds a refit round and the perturbation rounds below)
	constexpr uint32_t quality = WIDE ? 3u : (LEVEL == 1 ? 2u : (uint32_t)LEVEL);
	const uint32_t wt[4] = {kp.wt[0], kp.wt[1], kp.wt[2], kp.wt[3]};
	// fits with refit rounds start 1/16 inside the extremes (oracle: fitopt.start 1)
	constexpr float frac_main = iters ? 1.0f/16.0f : 0.0f;

	// a lane's best (error, id) so far live in words 18 / 19 of its column, like the payload fields: nothing of
	// a candidate is carried in registers from one trip of the stream loop to the next
	L_CSLOT[18*CF_WG_THREADS] = 0xFFFFFFFFu;
	L_CSLOT[19*CF_WG_THREADS] = 0x7FFFFFFFu;

	// ---- fit streams: one fit per lane (fit_lane) ----
	// Lowest / Low / Normal use the 32-lane layout (two blocks share a wave):
	//    hl  0..1  : mode 6, palette half = hl
	//    Normal: hl 2..5 / 6..9 : vector / scalar plane of mode 5, rotation hl-2 / hl-6
	//            hl 10..21 : mode 1, its 6 best partitions x 2 subsets; hl 22..31 : mode 3, 5 best
	//            (block with alpha: hl 10..31 : mode 7, its 11 best)
	//    Low:    Normal's layout, no refit round
	//    Lowest: hl 2 / 3 : mode 5 rotation 0 for blocks with alpha; no partitions
	// High and Highest use the 64-lane layout:
	// stream 0:  lanes  0..1  : mode 6
	//            lanes  2..13 : vector plane of candidate 1 + (lane-2) (mode 5 x rot, mode 4 x rot x isel)
	//            lanes 14..25 : scalar plane (rotated alpha) of candidate 1 + (lane-14)
	//            lanes 26..57 : two-subset partitions, 16 x 2 subsets: mode 7 with its 16 best
	//                           (blocks with alpha) or modes 1 + 3 with 8 each (High, opaque)
	// stream 1 (High, opaque blocks):
	//            lanes  0..29 : three-subset partitions, modes 0 + 2 with 5 partitions each
	// The partitions come from phase 1: every partition is scored once per subset count with
	// the residual estimator and the best are taken in (score, index) order.
	// Highest instead refits every partition (below), after a stream 0 without partitions.
	constexpr bool lay32 = !WIDE;
	// the first stream trip's fits get their integer statistics handed in ("moments handed in" below): the 32-lane
	// layouts.  The wide instances keep the row loop: with the hand-off Highest's linear build spills 5 vector registers.
	constexpr bool given = lay32;
#define L_HL (lay32 ? (lane & 31u) : lane)
#define L_SLOT_OK (!lay32 || pair || lane < 32u)
	constexpr uint32_t ntop = LEVEL >= 3 ? 8u : (LEVEL == 2 ? 4u : 1u);   // oracle: budget.top
	constexpr uint32_t uber = LEVEL >= 4 ? 2u : (LEVEL == 3 ? 1u : 0u);    // rounds per top candidate
	constexpr uint32_t uber2 = LEVEL >= 4 ? 2u : (LEVEL >= 2 ? 1u : 0u);   // rounds on the leader
	constexpr uint32_t msets = LEVEL >= 4 ? 3u : 1u;       // move sets of a round: bit 0 single, bit 1 joint (Highest only since round 6: oracle quality_budget)
	bool solved = false;
	// which halves walk the second pass: bit 0 / bit 32 = the best candidate of the first pass leaves the block
	// of half 0 / 1 with an error of at least 48 (oracle: best_err >= 48u); a scalar pair
	unsigned long long gb = 0ull;
#define H_GATE (((uint32_t)((pair && L_H) ? gb >> 32 : gb) & 1u) != 0u)
	// some half is opaque (the two-mode rankings are only walked then)
#define ANY_OPAQUE (pair ? (((uint32_t)abal & 0xFFFFu) == 0u || ((uint32_t)(abal >> 32) & 0xFFFFu) == 0u) : ((uint32_t)abal & 0xFFFFu) == 0u)
	{
		// second pass: the three-subset modes of an opaque block (Normal: mode 4 of an alpha-carrying one)
		// (the one budget value that stays a run-time scalar: with a constant trip count the compiler specialises the
		// loop by trip and holds more lane-role values across the fit -- the Normal build then spills a vector register)
		uint32_t nstreams = WIDE ? (has_alpha ? 1u : 2u) : (LEVEL == 2 ? 2u : 1u);
		asm volatile("" : "+s"(nstreams));
		// The last trip of this loop (sst) is not a stream of new candidates: it selects the `ntop` best so
		// far and refits them from four more starts (oracle: encode_block, "more starts") -- through the SAME
		// fit_lane call as the streams (one copy of the fit in the code object, one register allocation).
		constexpr uint32_t nsst = ntop > 4u ? 2u : 1u;       // four candidates per starts trip
#pragma unroll 1
		for (uint32_t st = 0; st < nstreams + nsst; ++st) {
			const bool sst = st >= nstreams;
			const uint32_t koff = sst ? (st - nstreams)*4u : 0u;
			if (!sst && solved)
				continue;
			CF_FRESH_LANE(lane);   // roles are recomputed per stream, not kept
			if (sst && koff == 0u) {
				// ---- the `ntop` best candidates of each group in (error, id) order (oracle: top[]) ----
				{
					typename CandKey<UNITW>::T kk = CandKey<UNITW>::make(L_CSLOT[18*CF_WG_THREADS], L_CSLOT[19*CF_WG_THREADS]);
					uint32_t wls = 0, wls2 = 0;          // byte k & 3 of word k >> 2: lane whose column holds the k-th best candidate
					for (uint32_t k = 0; k < ntop; ++k) {
						const typename CandKey<UNITW>::T km = CandKey<UNITW>::group_min(kk, pair, L_H);
						const unsigned long long bal = __ballot(kk == km);
						const uint32_t gmask = pair ? (L_H ? (uint32_t)(bal >> 32) : (uint32_t)bal) : 0u;
						const uint32_t wl = pair ? L_HBASE + (uint32_t)__ffs((int)gmask) - 1u
							: (uint32_t)__ffsll((long long)bal) - 1u;
						if (k < 4u) wls |= wl << (8u*k); else wls2 |= wl << (8u*(k - 4u));
						kk = lane == wl ? ~(typename CandKey<UNITW>::T)0 : kk;   // taken
					}
					L_CSLOT[20*CF_WG_THREADS] = wls;     // every lane keeps its group's list in its own column
					L_CSLOT[21*CF_WG_THREADS] = wls2;
				}
				if (uber2 == 0u || (CF_BC7_ABLATE & 16))
					break;
			}
			const Tex txp = make_tex(tile, plan, yccp, B_OFF, 0u, H_ALPHA ? 15u : 7u);   // partition fits: no rotation
			// the second pass of the 32-lane layout (s1l): slot s of an opaque half that walks it has its subsets
			// in lanes 11 + 2 s, 12 + 2 s and s; candidate 5 + k (mode 4) of an alpha-carrying half its vector /
			// scalar plane in lanes 11 + 2 k, 12 + 2 k -- the leaders are odd lanes from 11 up, whose columns no
			// candidate of the first pass uses (oracle: encode_block, "columns")
			const bool s1l = lay32 && st == 1u;
			// phase 1 is walked when some group ranks partitions in this trip
			const bool parts = quality >= 1u && !sst &&
				(!s1l || __ballot(L_SLOT_OK && !(H_ALPHA) && H_GATE) != 0ull);
			// A lane's roles are two words of k_bc7_roles (bc7_roles.h): the row is the half's (trip, alpha, second pass), the
			// column the lane of the half.  The address is an expression of a lane id re-read where a phase starts -- before
			// the fit, after the fit; phase 1's ranking forms it from the id re-read at the top of the trip, which phase 1
			// holds anyway -- and the words are dead where their phase ends: no role is carried in a register through the fit.
			// Lowest keeps the roles as expressions (below): its layout has four lanes with a role, which the compiler folds
			// to constants, and with the words it ran 1 % slower (profiles/lane_roles_bc7_ab.txt).
			constexpr bool words = quality != 0u;
			constexpr uint32_t rlay = WIDE ? CF_ROLE_LAY_WIDE : CF_ROLE_LAY_NORMAL;
			// (the rows of both halves are one wave-uniform word, a lane takes its half's byte: no branch on the lane id)
#define R_ROW (lay32 ? (role_rows32(st, abal, gb, pair) >> ((lane >> 2) & 8u)) & 7u : (st == 0u ? (uint32_t)(((uint32_t)abal & 0xFFFFu) != 0u) : 2u))
#define R_WORDS (k_bc7_roles.w + cf_bc7_role_index(rlay, R_ROW, L_HL))
			const uint32_t ns = 2u + st;     // subsets of this trip's partitions
			// The expression macros from here to R_RANK, and R_M6 .. R_IDBASE before the fit, serve the Lowest instances
			// alone (`!words`): in every other instance each use of them sits in a discarded `if constexpr` branch.
			// partition lanes: first lane, slots of the first mode, slots in all
			// (nper0 depends on the half's H_ALPHA: an expression, like the roles, not a carried value)
			const uint32_t pfirst = lay32 ? (quality == 2u ? 10u : 4u) : (st == 1u ? 0u : 26u);
			const uint32_t nslots = lay32 ? (quality == 2u ? 11u : 14u) : (st == 1u ? 10u : 16u);
#define R_NPER0 (st == 1u ? 5u : (lay32 ? (quality == 2u ? (H_ALPHA ? 11u : 6u) : 14u) : (H_ALPHA ? 16u : 12u)))
			// lane roles as expressions of the CURRENT lane id (re-read where a phase starts), so that none of
			// them is carried in a register through the fit
#define R_REL (L_HL - pfirst)                                   /* wraps below pfirst */
#define R_SLOT (s1l ? (L_HL < 10u ? L_HL : (L_HL - 11u) >> 1) : (st == 1u ? R_REL/3u : R_REL >> 1))
#define R_SUB (s1l ? (L_HL < 10u ? 2u : (L_HL - 11u) & 1u) : R_REL - R_SLOT*ns)
#define R_PLANE (parts && L_SLOT_OK && (s1l ? (!(H_ALPHA) && H_GATE && L_HL != 10u && L_HL != 31u) : (L_HL >= pfirst && R_SLOT < nslots)))
#define R_S1M4 (s1l && L_SLOT_OK && (H_ALPHA) && H_GATE && L_HL >= 11u && L_HL < 27u)
#define R_MI (R_SLOT >= R_NPER0 ? 1u : 0u)
#define R_RANK (R_SLOT - R_MI*R_NPER0)
			uint32_t mypart = 0;
			// ---- phase 1: partition scores (one partition per lane, two when the group has
			// only 32 lanes) and selection of the nper0 best by iterated group minimum ----
			if (parts) {
				// residual and scatter along the lines (oracle: partition_score) of the lane's partitions
				float sc0 = 0.0f, sl0 = 0.0f, sc1 = 0.0f, sl1 = 0.0f;
				const uint32_t npi = pair ? 2u : 1u;
				for (uint32_t pi = 0; pi < npi; ++pi) {
					const uint32_t part = pair ? L_HL + 32u*pi : lane;
					const uint32_t p2 = k_part2[part], p3 = k_part3[part];
					// one pass over the rows sums subset 1 (and 2); subset 0 is the block's table entry minus them
					const uint32_t m0 = st == 0u ? (~p2 & 0xFFFFu) : part3_mask(p3, 0u);
					const uint32_t m1 = st == 0u ? p2 : part3_mask(p3, 1u), m2 = st == 0u ? 0u : part3_mask(p3, 2u);
					Moments ma, mb;
					if (any_alpha) {
						if (st == 0u) moments_rows<true, false>(txp, m1, m2, ma, mb); else moments_rows<true, true>(txp, m1, m2, ma, mb);
					} else {
						if (st == 0u) moments_rows<false, false>(txp, m1, m2, ma, mb); else moments_rows<false, true>(txp, m1, m2, ma, mb);
					}
					// first stream trip: the owner of a partition leaves its subset-1 moments, packed like the block table,
					// where the lanes that fit the winning partitions find them (below, "moments handed in"): partition
					// lane + 32 pi in words 0..9 of the lane's candidate column (pi = 0) or fit-geometry column (pi = 1).
					// Both are dead here: no leader has stored a candidate of this block yet, and this trip's fits write
					// the geometry words after they have read these.  The geometry column's tag goes first, so that the
					// column cannot pass for a fit while it holds moments.
					if (given && st == 0u) {
						uint32_t* sc = (pi ? gbase : cbase) + lane;
						if (pi)
							sc[12*CF_WG_THREADS] = CF_BC7_GEO_NONE;
						sc[0*CF_WG_THREADS] = ma.q00 | (ma.s[0] << 20); sc[1*CF_WG_THREADS] = ma.q11 | (ma.s[1] << 20);
						sc[2*CF_WG_THREADS] = ma.q22 | (ma.s[2] << 20); sc[3*CF_WG_THREADS] = ma.q33 | (ma.s[3] << 20);
						sc[4*CF_WG_THREADS] = ma.q01; sc[5*CF_WG_THREADS] = ma.q02; sc[6*CF_WG_THREADS] = ma.q03;
						sc[7*CF_WG_THREADS] = ma.q12; sc[8*CF_WG_THREADS] = ma.q13; sc[9*CF_WG_THREADS] = ma.q23;
					}
					// subsets 0, 1 (, 2) in the oracle's order of summation
					float sc = 0.0f, sl = 0.0f, al;
					{
						const uint32_t* tw = mom + (txp.boff >> 4)*CF_BC7_MOM_WORDS;
						if (any_alpha) {
							const Moments m0s = st == 0u ? moments_rest<true, false>(tw, ma, mb) : moments_rest<true, true>(tw, ma, mb);
							sc = sc + subset_residual<true>(m0s, m0, al);
						} else {
							const Moments m0s = st == 0u ? moments_rest<false, false>(tw, ma, mb) : moments_rest<false, true>(tw, ma, mb);
							sc = sc + subset_residual<false>(m0s, m0, al);
						}
						sl = sl + al;
					}
					sc = sc + (any_alpha ? subset_residual<true>(ma, m1, al) : subset_residual<false>(ma, m1, al));
					sl = sl + al;
					if (st != 0u) {
						sc = sc + (any_alpha ? subset_residual<true>(mb, m2, al) : subset_residual<false>(mb, m2, al));
						sl = sl + al;
					}
					if (pi == 0u) { sc0 = sc; sl0 = sl; } else { sc1 = sc; sl1 = sl; }
				}
				// one ranking per mode of the group: modes 1 / 3 (alpha: mode 7 alone), modes 0 / 2; key = bits of
				// residual + along / (4 (2^ib)^2), low 6 bits = the partition (oracle: encode_block, "qf")
				const uint32_t nruns = (st == 1u || ANY_OPAQUE) ? 2u : 1u;
				// the slot this lane fits: mi | rank << 1 of its role word (no partition lane: a rank no selection reaches)
				static_assert(CF_ROLE_NO_RANK >= 16u, "no selection below (at most 16 per run) may reach the rank of a lane that fits no subset");
				const uint32_t rankmi = words ? CF_ROLE_RANKMI(R_WORDS[0]) : ((R_RANK << 1) | R_MI);
				for (uint32_t run = 0; run < nruns; ++run) {
					CF_FRESH_LANE(lane);
					// (formed here from its bits: as a float select it is hoisted out of the stream loop and held in a register)
					uint32_t qfb = (run == 0u && !(st == 0u && (H_ALPHA))) ? 0x3C000000u : 0x3D000000u;   // 1/128 : 1/32
					asm volatile("" : "+v"(qfb));
					const float qf = __uint_as_float(qfb);
					const uint32_t part0 = pair ? L_HL : lane;
					const uint32_t npart = (st == 1u && run == 0u) ? 16u : 64u;   // mode 0 ranks its own 16 partitions
					uint32_t ka = part0 < npart ? ((__float_as_uint(fmaf(qf, sl0, sc0)) & ~63u) | part0) : 0xFFFFFFFFu;
					uint32_t kb = (pair && npart == 64u) ? ((__float_as_uint(fmaf(qf, sl1, sc1)) & ~63u) | (part0 + 32u)) : 0xFFFFFFFFu;
					// uniform trip count: the larger of the groups' needs
					const uint32_t nsel = st == 1u ? 5u : (run == 0u ? (lay32 ? (quality == 2u ? (any_alpha ? 11u : 6u) : 14u) : (has_alpha ? 16u : 12u))
						: (lay32 ? 5u : 4u));
					for (uint32_t t = 0; t < nsel; ++t) {
						const uint32_t kmin = cf_group_min_u32(ka < kb ? ka : kb, pair, L_H);
						const bool mine = rankmi == ((t << 1) | run);
						mypart = mine ? (kmin & 63u) : mypart;
						ka = ka == kmin ? 0xFFFFFFFFu : ka;
						kb = kb == kmin ? 0xFFFFFFFFu : kb;
					}
				}
			}
			// ---- lane roles ----
			if (given)
				__builtin_amdgcn_wave_barrier();   // the moments phase 1 left in LDS are read below
			CF_FRESH_LANE(lane);
			asm volatile("" : "+v"(mypart));   // nothing of phase 1 but mypart lives on
#define R_M6 (st == 0u && L_SLOT_OK && L_HL < 2u)
#define R_VECP (lay32 ? (st == 1u ? (R_S1M4 && ((L_HL - 11u) & 1u) == 0u) : (quality == 2u ? (L_SLOT_OK && L_HL >= 2u && L_HL < 6u) : (L_SLOT_OK && L_HL == 2u))) : (st == 0u && lane >= 2u && lane < 14u))
#define R_SCA (lay32 ? (st == 1u ? (R_S1M4 && ((L_HL - 11u) & 1u) != 0u) : (quality == 2u ? (L_SLOT_OK && L_HL >= 6u && L_HL < 10u) : (L_SLOT_OK && L_HL == 3u))) : (st == 0u && lane >= 14u && lane < 26u))
#define R_CID (R_M6 ? 0u : (lay32 ? (st == 1u ? 5u + ((L_HL - 11u) >> 1) : (quality == 2u ? L_HL - (R_SCA ? 5u : 1u) : 1u)) : 1u + (lane - (R_SCA ? 14u : 2u))))   /* meaningful for vecp / sca */
#define R_IDBASE (R_PLANE ? (st == 1u ? (R_MI ? 256u : 192u) : (H_ALPHA ? 320u : (R_MI ? 128u : 64u))) : 0u)
			bool m6 = false, sca = false, vecp = false, plane = false;
			uint32_t cid = 0, sub = 0, mi = 0;
			if constexpr (!words) {
				m6 = R_M6; sca = R_SCA; vecp = R_VECP; plane = R_PLANE;
				cid = R_CID; sub = R_SUB; mi = R_MI;
			}
			const uint32_t s2off = lay32 ? ((quality == 2u && st == 0u) ? 4u : 1u) : (st == 0u ? 12u : 2u);   // (read by the assembly on the expressions alone)
			uint32_t rot = 0, cb = 7, ab = 7, pbk = 1, ib = 4, mask = 0xFFFFu;
			bool active = m6;
			float frac = frac_main;
			uint32_t chm_s = 0;
			uint32_t gmode = 1u, gsrc = 0u;   // stream trips write the fit-geometry cache, the starts trip reads it
			bool narrow = false;              // starts trip: no active lane's fit has more than 4 palette entries
			bool whole = true;                // the fit covers the whole block (its search bias: fit_lane); set below
			if (sst) {
				// lane = (top candidate k, start variant v, fit): 8 lanes per candidate in the 32-lane layouts
				// (k = hl >> 3, v = (hl >> 1) & 3, fit = hl & 1 -- mode 6: its two palette halves), 16 in the wide
				// one (k = lane >> 4, v = (lane >> 2) & 3, fit = lane & 3).  Each lane runs the whole fit from its
				// start; the best start of a fit replaces the column's fit when it is better.
				// A three-subset candidate has 8 lanes in the 32-lane layout as well: two starts (v = 0, 1: the extremes,
				// pushed out) of its three fits in j = hl & 7 = 3 v + fit, j < 6 (oracle: budget.starts3)
				const uint32_t k = koff + (lay32 ? (L_HL >> 3) : (lane >> 4));
				const uint32_t wl = TOP_LANE(k & 7u);
				const uint32_t id = cbase[wl + 19*CF_WG_THREADS], cerr = cbase[wl + 18*CF_WG_THREADS];
				// (three subsets, from the candidate word: ids 192 .. 319)
				const bool n3 = lay32 && CF_CAND_NS(cbase[wl + 6*CF_WG_THREADS]) == 3u;
				const uint32_t j8 = L_HL & 7u;
				const uint32_t v = lay32 ? (n3 ? (j8 >= 3u ? 1u : 0u) : (L_HL >> 1) & 3u) : (lane >> 2) & 3u;
				const uint32_t fi = lay32 ? (n3 ? (j8 >= 6u ? 3u : j8 - 3u*v) : (L_HL & 1u)) : (lane & 3u);
				const uint32_t err0 = cbase[TOP_LANE(0u) + 18*CF_WG_THREADS];
				const FitGeo g = column_geo(cbase + wl, id, fi);
				m6 = g.m6; sca = g.sca; rot = g.rot; cb = g.cb; ab = g.ab; pbk = g.pbk; ib = g.ib; mask = g.mask;
				chm_s = g.chm;
				if constexpr (UNITW) whole = g.ns < 2u;   // one subset: mode 6, the planes of modes 4 / 5
				active = L_SLOT_OK && k < ntop && cerr != 0xFFFFFFFFu && err0 != 0u && (g.m6 ? fi < 2u : fi < g.nfits);
				// starts 0, 2, 3, 4 of the oracle: the extremes, pushed out by 1/16, pulled in by 1/8, by 3/16
				frac = v == 0u ? 0.0f : (v == 1u ? -1.0f/16.0f : (v == 2u ? 1.0f/8.0f : 3.0f/16.0f));
				// parts A and B of the fit come from the cache when every active lane of the wave finds its fit there
				// (in its own block's half); otherwise the whole wave computes them
				gsrc = geo_src(g, fi, wl, lay32);
				const bool ghit = gbase[gsrc + 12*CF_WG_THREADS] == geo_tag(g, id, fi) && (!lay32 || ((gsrc ^ wl) & 32u) == 0u);
				gmode = __ballot(active && !ghit) == 0ull ? 2u : 0u;
				narrow = __ballot(active && (g.m6 || g.ib > 2u)) == 0ull;
				CF_DIAG_COUNT(CF_DIAG_STARTS, true);
				CF_DIAG_COUNT(CF_DIAG_STARTS_CACHED, gmode == 2u);
				CF_DIAG_COUNT(CF_DIAG_STARTS_NARROW, narrow);
			} else if constexpr (words) {
				const uint32_t* rp = R_WORDS;   // (one address, one two-word load)
				const uint32_t rw = rp[0], fw = rp[1];
				m6 = (rw & CF_ROLE_M6) != 0u; sca = (rw & CF_ROLE_SCA) != 0u; plane = (rw & CF_ROLE_PLANE) != 0u;
				sub = CF_ROLE_KF(rw);
				active = CF_ROLE_ACTIVE(rw, UNITW) != 0u;
				rot = CF_FIT_ROT(fw); chm_s = CF_FIT_CHM(fw);
				cb = CF_FIT_GEO(fw) & 15u; ab = (CF_FIT_GEO(fw) >> 4) & 15u; pbk = (CF_FIT_GEO(fw) >> 8) & 15u; ib = CF_FIT_GEO(fw) >> 12;
				// a subset's texels (mypart is 0 on every other lane: a valid index, and the whole block is its mask)
				const uint32_t sp2 = k_part2[mypart], sp3 = k_part3[mypart];
				const uint32_t smask = st == 0u ? (sub ? sp2 : (~sp2 & 0xFFFFu)) : part3_mask(sp3, sub);
				mask = plane ? smask : 0xFFFFu;
			} else if (vecp || sca) {
				if (cid <= 4u) {
					rot = cid - 1u; pbk = 0; ib = 2;
					cb = sca ? 0u : 7u; ab = sca ? 8u : 0u;
					active = quality >= 2u || (quality == 1u ? cid == 1u : (cid == 1u && H_ALPHA));
					// the perceptual metric couples R, G and B: no plane split that moves a colour
					// channel into the scalar plane (oracle: nrot)
					active = active && (UNITW || rot == 0u);
				} else {
					const uint32_t isel = (cid - 5u) >> 2;
					rot = (cid - 5u) & 3u; pbk = 0;
					cb = sca ? 0u : 5u; ab = sca ? 6u : 0u;
					ib = (isel != 0u) == sca ? 2u : 3u;   // isel 0: 2-bit colour / 3-bit alpha indices
					active = quality >= 2u && (UNITW || rot == 0u);     // (mode 4 exists only in the 64-lane layout: Highest)
				}
			} else if (plane) {
				uint32_t mode;
				if (st == 1u) mode = mi ? 2u : 0u;
				else mode = H_ALPHA ? 7u : (mi ? 3u : 1u);
				switch (mode) {
					case 1: cb = 6; ab = 0; pbk = 2; ib = 3; break;
					case 3: cb = 7; ab = 0; pbk = 1; ib = 2; break;
					case 0: cb = 4; ab = 0; pbk = 1; ib = 3; break;
					case 2: cb = 5; ab = 0; pbk = 0; ib = 2; break;
					default: cb = 5; ab = 5; pbk = 1; ib = 2; break;
				}
				const uint32_t sp2 = k_part2[mypart], sp3 = k_part3[mypart];
				if (st == 0u)
					mask = sub ? sp2 : (~sp2 & 0xFFFFu);
				else
					mask = part3_mask(sp3, sub);
				active = true;
			}
			if constexpr (UNITW) {
				if (!sst) whole = !plane;
			}
			if (CF_BC7_ABLATE & 1) active = active && (m6 || plane);
			if (CF_BC7_ABLATE & 2) active = active && !plane;
#if CF_BC7_DIAG
			const bool nopb = __ballot(active && pbk != 0u) == 0ull;   // (a ballot of the whole wave: outside the counter's lane test)
			CF_DIAG_COUNT(CF_DIAG_STARTS_NOPB, sst && nopb);
#endif
			uint32_t wl[4] = {wt[0], wt[1], wt[2], wt[3]};
			if (!UNITW && rot) {
				const uint32_t t3 = wl[3];
				if (rot == 1u) { wl[3] = wl[0]; wl[0] = t3; }
				else if (rot == 2u) { wl[3] = wl[1]; wl[1] = t3; }
				else { wl[3] = wl[2]; wl[2] = t3; }
			}
			// channels this fit codes (after rotation) and their weights
			const uint32_t chm = (sst || words) ? chm_s : (m6 ? 15u : (sca ? 8u : (vecp ? 7u : (H_ALPHA ? 15u : 7u))));
			const uint32_t wv[4] = {(chm & 1u) ? wl[0] : 0u, (chm & 2u) ? wl[1] : 0u,
				(chm & 4u) ? wl[2] : 0u, (chm & 8u) ? wl[3] : 0u};
			LaneFit lf;
			lf.err = 0; lf.q0 = 0; lf.q1 = 0; lf.pb = 0;
#pragma unroll
			for (int k = 0; k < 4; ++k) lf.w[k] = 0;
			// perceptual weight pairs of this fit: zero on the axes it does not code
			const uint32_t yw[2] = {(chm & 7u) ? ywrg : 0u,
				((chm & 7u) ? (ywba & 0xFFFFu) : 0u) | ((chm & 8u) ? (ywba & 0xFFFF0000u) : 0u)};
			// ---- moments handed in: in the first stream trip every fit's integer statistics exist already ----
			// mode 6 and the planes of modes 4 / 5 fit the whole block: the block table's words in the fit's channel slots
			// (mom_whole), the extremes of its rotated alpha from the table of channel extremes.  A partition lane takes the
			// subset-1 moments its partition's owner left in LDS (phase 1); subset 0 is the block minus them, as in
			// moments_rest.  The later trips keep the row loop: the second pass, whose candidate columns are live, and the
			// starts trip where the cache misses.
			FitStats gs;   // (filled, and read by the fit, in the first stream trip alone)
			if (given && st == 0u) {
				const uint32_t blk = B_OFF >> 4;
				uint32_t T[CF_MOM_WORDS];
#pragma unroll
				for (int m = 0; m < CF_MOM_WORDS; ++m) T[m] = mom[__umul24(blk, CF_BC7_MOM_WORDS) + (uint32_t)m];
				gs.lohi = lohi[blk*4u + ((rot + 3u) & 3u)];
				// (branches on the lane's role, not selects: under the execution mask a subset-1 lane's words are loaded
				// straight into place and only the subset-0 lanes' subtraction and the whole-block lanes' derivation issue)
				if (quality >= 1u && plane) {
					// owner of partition p: lane p & 31 of the half, word set p >> 5 (one block per wave: lane p)
					const uint32_t* sc = ((pair && mypart >= 32u) ? gbase : cbase) + (pair ? L_HBASE + (mypart & 31u) : mypart);
#pragma unroll
					for (int m = 0; m < CF_MOM_WORDS; ++m) gs.W[m] = sc[m*CF_WG_THREADS];
					if (sub == 0u) {
						mom_sub(T, gs.W, gs.W);
						asm volatile("" : "+v"(gs.W[0]));   // (keeps this a branch: as a select every lane pays for both forms)
					}
				} else
					mom_whole(T, !(H_ALPHA), rot, chm, gs.W);
				__builtin_amdgcn_wave_barrier();   // read before any fit writes its geometry words
				gmode = 3u;
			}
			// Matrix pipe: v_mfma takes a row's texels from lanes 32h + 0..3 and gives wrong results when lanes are switched off
			// (tools/ubench/mfma_layout.hip), so the fit runs with the whole wave on whenever any lane has one.  A lane without
			// a fit walks it on its role row's defaults, stores nothing (owner) and its result is cleared below.
			if (UNITW ? __ballot(active) != 0ull : active) {
				if (narrow)
					fit_lane<UNITW, iters, 4, false, WIDE ? 4 : 3>(make_tex(tile, plan, yccp, B_OFF, rot, chm), mask, m6, lane & 1u, cb, ab, pbk, ib,
						wv, yw, sca, frac, gbase, gmode, gsrc, gs, active, whole, lohi, lf);
				else
					fit_lane<UNITW, iters, 8, given, WIDE ? 4 : 3>(make_tex(tile, plan, yccp, B_OFF, rot, chm), mask, m6, lane & 1u, cb, ab, pbk, ib,
						wv, yw, sca, frac, gbase, gmode, gsrc, gs, active, whole, lohi, lf);
				if (UNITW && !active) {
					lf.err = 0; lf.q0 = 0; lf.q1 = 0; lf.pb = 0;
#pragma unroll
					for (int k = 0; k < 4; ++k) lf.w[k] = 0;
				}
			}
			CF_FRESH_LANE(lane);         // the roles below are computed again from here
			if (sst) {
				// (every role again from the fresh lane id: nothing but the fit's result lived across fit_lane)
				const uint32_t k2 = koff + (lay32 ? (L_HL >> 3) : (lane >> 4));
				const uint32_t wl2 = TOP_LANE(k2 & 7u);
				const uint32_t id2 = cbase[wl2 + 19*CF_WG_THREADS], cerr2 = cbase[wl2 + 18*CF_WG_THREADS];
				const bool n32 = lay32 && CF_CAND_NS(cbase[wl2 + 6*CF_WG_THREADS]) == 3u;
				const uint32_t j82 = L_HL & 7u;
				const uint32_t v2 = lay32 ? (n32 ? (j82 >= 3u ? 1u : 0u) : (L_HL >> 1) & 3u) : (lane >> 2) & 3u;
				const uint32_t fi2 = lay32 ? (n32 ? (j82 >= 6u ? 3u : j82 - 3u*v2) : (L_HL & 1u)) : (lane & 3u);
				const uint32_t err02 = cbase[TOP_LANE(0u) + 18*CF_WG_THREADS];
				const FitGeo g2 = column_geo(cbase + wl2, id2, fi2);
				const uint32_t kf2 = g2.m6 ? 0u : fi2;
				const bool active2 = L_SLOT_OK && k2 < ntop && cerr2 != 0xFFFFFFFFu && err02 != 0u && (g2.m6 ? fi2 < 2u : fi2 < g2.nfits);
				// best start of the fit: minimum of (error, v) over the four lanes of (k, fit)
				uint32_t skey = active2 ? ((lf.err << 2) | v2) : 0xFFFFFFFFu;
				{
					// (three fits in 8 lanes: the other start of the fit is 3 lanes away; lanes 6, 7 idle)
					const uint32_t o1 = (uint32_t)cf_bperm((int)skey, n32 ? (j82 < 3u ? lane + 3u : (j82 < 6u ? lane - 3u : lane)) : lane ^ (lay32 ? 2u : 4u));
					skey = o1 < skey ? o1 : skey;
					const uint32_t o2 = (uint32_t)cf_bperm((int)skey, n32 ? lane : lane ^ (lay32 ? 4u : 8u));
					skey = o2 < skey ? o2 : skey;
				}
				uint32_t* wc = cbase + wl2;
				const uint32_t cur_err = wc[(15u + kf2)*CF_WG_THREADS];
				const bool win = active2 && skey == ((lf.err << 2) | v2) && lf.err < cur_err && (!g2.m6 || fi2 == 0u);
				// every fit at once: the fits of a candidate share the weight words of its column, and each puts its own
				// bytes there by and / or (column_put_fit); the p-bit word one fit at a time
				if (win)
					column_put_fit(wc, g2, kf2, lf.q0, lf.q1, lf.w, lf.err);
#pragma unroll 1
				for (uint32_t j = 0; j < 3u; ++j) {
					if (win && !g2.planes45 && kf2 == j)
						column_put_pbits(wc, kf2, lf.pb);
					__builtin_amdgcn_wave_barrier();
				}
				continue;
			}
			uint32_t best_err;
			if constexpr (words) {
				// ---- assemble candidates in their leader lanes: straight-line code on the lane's role word ----
				//   mode 6: its first lane;  mode 4/5: vector lane (scalar plane in lane s2);
				//   partitions: subset-0 lane (subset 1 in the next lane, subset 2 in lane s2)
				const uint32_t rw = R_WORDS[0];
				bool act = CF_ROLE_ACTIVE(rw, UNITW) != 0u;
				if (CF_BC7_ABLATE & 1) act = act && (rw & (CF_ROLE_M6 | CF_ROLE_PLANE)) != 0u;
				if (CF_BC7_ABLATE & 2) act = act && (rw & CF_ROLE_PLANE) == 0u;
				// the candidate of this lane's fit (a lane that fits no subset has ranked no partition: mypart is 0)
				const uint32_t cidv = CF_ROLE_IDB(rw) + mypart;
				// the fit this lane's geometry-cache column now holds: written by every lane of the first stream trip (a
				// column of the previous block must not pass for this one's), by the lanes that ran a fit in a later one
				if (act || st == 0u)
					gbase[lane + 12*CF_WG_THREADS] = act ? cidv*4u + CF_ROLE_KF(rw) : CF_BC7_GEO_NONE;   // geo_tag (mode 6: fit 0)
				const uint32_t s1 = (lane + 1u) & 63u;
				const uint32_t s2 = (lay32 ? (lane & 32u) : 0u) + CF_ROLE_S2(rw);
				// which gathered fits belong to this lane's candidate, as masks: subset 1 (use1: every partition), the scalar
				// plane (vector lanes), subset 2 (the second pass's partitions: use2 of a lane that is no vector plane)
				const uint32_t m1 = 0u - CF_ROLE_USE1(rw), mv = 0u - ((rw / CF_ROLE_VECP) & 1u), m2 = 0u - CF_ROLE_USE2(rw);
				const uint32_t m3 = m2 & ~mv, m4 = (mv & 0xFF000000u) | m3;
				const uint32_t e1 = (uint32_t)cf_bperm((int)lf.err, s1), e2 = (uint32_t)cf_bperm((int)lf.err, s2);
				const uint32_t a01 = (uint32_t)cf_bperm((int)lf.q0, s1), a11 = (uint32_t)cf_bperm((int)lf.q1, s1);
				const uint32_t a02 = (uint32_t)cf_bperm((int)lf.q0, s2), a12 = (uint32_t)cf_bperm((int)lf.q1, s2);
				const uint32_t pb1 = (uint32_t)cf_bperm((int)lf.pb, s1), pb2 = (uint32_t)cf_bperm((int)lf.pb, s2);
				uint32_t w1[4], w2[4];
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					w1[k] = (uint32_t)cf_bperm((int)lf.w[k], s1);
					w2[k] = (uint32_t)cf_bperm((int)lf.w[k], s2);
				}
				// only a leader whose candidate beats its best so far stores the payload fields into its LDS column
				const uint32_t cerr = lf.err + (e1 & m1) + (e2 & m2);
				const bool leader = act && CF_ROLE_LEADER(rw) != 0u;
				const uint32_t old_err = L_CSLOT[18*CF_WG_THREADS], old_id = L_CSLOT[19*CF_WG_THREADS];
				// (error, id) order as one 64-bit comparison
				const bool take = leader & ((((unsigned long long)cerr << 32) | cidv) < (((unsigned long long)old_err << 32) | old_id));
				best_err = take ? cerr : old_err;
				if (take) {
					L_CSLOT[18*CF_WG_THREADS] = cerr;
					L_CSLOT[19*CF_WG_THREADS] = cidv;
					L_CSLOT[0*CF_WG_THREADS] = lf.q0;
					L_CSLOT[1*CF_WG_THREADS] = lf.q1;
					L_CSLOT[2*CF_WG_THREADS] = a01 & m1;
					L_CSLOT[3*CF_WG_THREADS] = a11 & m1;
					// modes 4/5: the scalar plane's endpoints are parked in q[4], q[5] (byte 3)
					L_CSLOT[4*CF_WG_THREADS] = a02 & m4;
					L_CSLOT[5*CF_WG_THREADS] = a12 & m4;
					// the p-bits, and above them what the candidate is (bc7_cand.h): no later phase decodes it from its id
					// (stored where it is read: the levels that come back to their candidates, Normal and up)
					L_CSLOT[6*CF_WG_THREADS] = lf.pb | ((pb1 << 2) & m1) | ((pb2 << 4) & m3) | (uber2 ? k_bc7_cands.w[cf_bc7_cand_index(cidv)] : 0u);
					// errors of the candidate's fits: subset 0 / vector plane / mode 6, then subset 1 or
					// the scalar plane, then subset 2
					L_CSLOT[15*CF_WG_THREADS] = lf.err;
					L_CSLOT[16*CF_WG_THREADS] = (e1 & m1) | (e2 & mv);
					L_CSLOT[17*CF_WG_THREADS] = e2 & m3;
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						L_CSLOT[(7 + k)*CF_WG_THREADS] = lf.w[k] | (w1[k] & m1) | (w2[k] & m3);
						L_CSLOT[(11 + k)*CF_WG_THREADS] = w2[k] & mv;
					}
				}
			} else {
				// Lowest: the assembly on the role expressions, its gathers and stores behind the branches on them
				// the fit this lane's geometry-cache column now holds: written by every lane of the first stream trip (a
				// column of the previous block must not pass for this one's), by the lanes that ran a fit in a later one
				if (active || st == 0u)
					gbase[lane + 12*CF_WG_THREADS] = active ? geo_tag(R_M6 ? 0u : ((R_VECP || R_SCA) ? R_CID : R_IDBASE + mypart),
						R_SCA ? 1u : (R_PLANE ? R_SUB : 0u)) : CF_BC7_GEO_NONE;
				// ---- assemble candidates in their leader lanes ----
				//   mode 6: its first lane;  mode 4/5: vector lane (scalar plane s2off lanes up);
				//   partitions: subset-0 lane (the other subsets in the next lanes)
				const int s1 = (int)((lane + 1u) & 63u);
				const int s2 = (s1l && R_PLANE) ? (int)(L_HBASE + ((L_HL - 11u) >> 1)) : (int)((lane + s2off) & 63u);
				// error and id first: only a leader whose candidate beats its best so far stores
				// the payload fields, straight from the shuffles into its LDS column
				const uint32_t e1 = (uint32_t)cf_bperm((int)lf.err, (uint32_t)(s1)), e2 = (uint32_t)cf_bperm((int)lf.err, (uint32_t)(s2));
				const bool use1 = R_PLANE, use2 = R_VECP || (R_PLANE && st == 1u);
				const uint32_t cerr = lf.err + (use1 ? e1 : 0u) + (use2 ? e2 : 0u);
				const uint32_t cidv = R_M6 ? 0u : (R_VECP ? R_CID : R_IDBASE + mypart);
				const bool leader = active && (R_M6 ? L_HL == 0u : (R_VECP || (R_PLANE && R_SUB == 0u)));
				const uint32_t old_err = L_CSLOT[18*CF_WG_THREADS], old_id = L_CSLOT[19*CF_WG_THREADS];
				const bool take = leader && (cerr < old_err || (cerr == old_err && cidv < old_id));
				best_err = take ? cerr : old_err;
				if (take) {
					L_CSLOT[18*CF_WG_THREADS] = cerr;
					L_CSLOT[19*CF_WG_THREADS] = cidv;
				}
				{
					const uint32_t a01 = (uint32_t)cf_bperm((int)lf.q0, (uint32_t)(s1)), a11 = (uint32_t)cf_bperm((int)lf.q1, (uint32_t)(s1));
					const uint32_t a02 = (uint32_t)cf_bperm((int)lf.q0, (uint32_t)(s2)), a12 = (uint32_t)cf_bperm((int)lf.q1, (uint32_t)(s2));
					const uint32_t pb1 = (uint32_t)cf_bperm((int)lf.pb, (uint32_t)(s1)), pb2 = (uint32_t)cf_bperm((int)lf.pb, (uint32_t)(s2));
					if (take) {
						L_CSLOT[0*CF_WG_THREADS] = lf.q0;
						L_CSLOT[1*CF_WG_THREADS] = lf.q1;
						L_CSLOT[2*CF_WG_THREADS] = R_PLANE ? a01 : 0u;
						L_CSLOT[3*CF_WG_THREADS] = R_PLANE ? a11 : 0u;
						// modes 4/5: the scalar plane's endpoints are parked in q[4], q[5] (byte 3)
						L_CSLOT[4*CF_WG_THREADS] = R_VECP ? (a02 & 0xFF000000u) : ((R_PLANE && st == 1u) ? a02 : 0u);
						L_CSLOT[5*CF_WG_THREADS] = R_VECP ? (a12 & 0xFF000000u) : ((R_PLANE && st == 1u) ? a12 : 0u);
						L_CSLOT[6*CF_WG_THREADS] = lf.pb | (R_PLANE ? (pb1 << 2) : 0u) |
							((R_PLANE && st == 1u) ? (pb2 << 4) : 0u);
						// errors of the candidate's fits: subset 0 / vector plane / mode 6, then subset 1 or
						// the scalar plane, then subset 2
						L_CSLOT[15*CF_WG_THREADS] = lf.err;
						L_CSLOT[16*CF_WG_THREADS] = R_PLANE ? e1 : (R_VECP ? e2 : 0u);
						L_CSLOT[17*CF_WG_THREADS] = (R_PLANE && st == 1u) ? e2 : 0u;
					}
				}
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					const uint32_t w1 = (uint32_t)cf_bperm((int)lf.w[k], (uint32_t)(s1));
					const uint32_t w2 = (uint32_t)cf_bperm((int)lf.w[k], (uint32_t)(s2));
					if (take) {
						L_CSLOT[(7 + k)*CF_WG_THREADS] = lf.w[k] | (R_PLANE ? w1 : 0u) |
							((R_PLANE && st == 1u) ? w2 : 0u);
						L_CSLOT[(11 + k)*CF_WG_THREADS] = R_VECP ? w2 : 0u;
					}
				}
			}
			// A zero-error candidate cannot be beaten by a later one (ids grow with the
			// streams), so the remaining work may be skipped without changing the payload.
			// The second pass only for blocks whose best candidate so far leaves an error of at least 48 (oracle:
			// same rule; a zero-error block ends its search here): per half, and skipped when no half walks it
			if (st == 0u) {
				const uint32_t gmin = cf_group_min_u32(best_err, pair, L_H);
				gb = __ballot(gmin >= (UNITW ? 48u : 256u));     // oracle: gate2
				solved = gb == 0ull;
			}
#undef R_ROW
#undef R_WORDS
#undef R_NPER0
#undef R_REL
#undef R_SLOT
#undef R_SUB
#undef R_PLANE
#undef R_MI
#undef R_RANK
#undef R_M6
#undef R_VECP
#undef R_SCA
#undef R_CID
#undef R_IDBASE
#undef R_S1M4
		}
	}

	// ---- the `ntop` best candidates of each group in (error, id) order (oracle: top[]) ----
	// From Normal up the best candidates are refined before one of them wins: refitted from four more
	// starts (every fit keeps its best), perturbed for `uber` rounds each, and the best of them then for
	// `uber2` more rounds.  Lowest / Low: ntop = 1, no refinement, the argmin packs.
	CF_FRESH_LANE(lane);
	uint32_t win_lane = TOP_LANE(0u);

	if (uber2) {
		// the lanes that own a refined column take its new total
		CF_FRESH_LANE(lane);
		{
			bool own = false;
			for (uint32_t k = 0; k < ntop; ++k)
				own = own || lane == TOP_LANE(k);
			if (own && L_CSLOT[18*CF_WG_THREADS] != 0xFFFFFFFFu)
				L_CSLOT[18*CF_WG_THREADS] = L_CSLOT[15*CF_WG_THREADS] + L_CSLOT[16*CF_WG_THREADS] + L_CSLOT[17*CF_WG_THREADS];
			__builtin_amdgcn_wave_barrier();
		}

		// ---- endpoint perturbation (oracle: uber_refine) of every top candidate, then of the leader ----
		// lane = (fit of the candidate, move slot): 16 slots per fit and move set -- set 0: endpoint m >> 3,
		// channel (m >> 1) & 3, direction m & 1: +-1 on that quantised field, the slots of a channel the fit
		// does not code flip p-bits; set 1: channel m >> 2, both ends of it by (+1,+1), (-1,-1), (+1,-1), (-1,+1)
		// -- scored by the exhaustive selector assignment; per fit (= per DPP row of 16 lanes; mode 6 spreads
		// its 16 palette entries over lane pairs and fills two rows) the best move of a set is applied when it
		// lowers the fit's error; a round walks its sets in order.  Fits are independent, so all of them move
		// in the same pass.
		// In the 32-lane layout a block has two rows of move slots, so the third fit of a three-subset candidate
		// gets a pass of its own (fp = 1: fits 2 and 3) -- fits are independent, and one that did not move in a round
		// never moves again, so fit 2 walking its rounds after fits 0 and 1 ends where the oracle's round-major order does.
#pragma unroll 1
		for (uint32_t kf2p = ((CF_BC7_ABLATE & 32) || !uber) ? 2u*ntop : 0u; kf2p <= 2u*ntop + 1u; ++kf2p) {
			const uint32_t kk = kf2p >> 1, fp = kf2p & 1u;
			CF_FRESH_LANE(lane);
			uint32_t wl = (fp && kk == ntop) ? win_lane : TOP_LANE(kk & 7u);
			if (fp) {
				// a second pass only when a candidate of this wave has a third fit (ids 192 .. 319: modes 0 and 2)
				const uint32_t idf = cbase[wl + 19*CF_WG_THREADS];
				if (!lay32 || __ballot(L_SLOT_OK && idf >= 192u && idf < 320u) == 0ull)
					continue;
			}
			if (kk == ntop && !fp) {
				// the leader after the candidates' own rounds
				const typename CandKey<UNITW>::T key = CandKey<UNITW>::make(L_CSLOT[18*CF_WG_THREADS], L_CSLOT[19*CF_WG_THREADS]);
				const typename CandKey<UNITW>::T kmin = CandKey<UNITW>::group_min(key, pair, L_H);
				const unsigned long long bal = __ballot(key == kmin);
				const uint32_t gmask = pair ? (L_H ? (uint32_t)(bal >> 32) : (uint32_t)bal) : 0u;
				wl = pair ? L_HBASE + (uint32_t)__ffs((int)gmask) - 1u : (uint32_t)__ffsll((long long)bal) - 1u;
				win_lane = wl;
			}
			uint32_t* wc = cbase + wl;
			const uint32_t id = wc[19*CF_WG_THREADS], cerr = wc[18*CF_WG_THREADS];
			const uint32_t kf0 = (L_HL >> 4) + 2u*fp;
			const FitGeo g0 = column_geo(wc, id, kf0);
			const uint32_t kf = g0.m6 ? 0u : kf0, mv = g0.m6 ? (L_HL >> 1) & 15u : (L_HL & 15u);
			const FitGeo g = g0;
			const bool act = L_SLOT_OK && L_HL < 64u && (g.m6 ? (L_HL < 32u && !fp) : kf < g.nfits) && cerr != 0u && cerr != 0xFFFFFFFFu;
			const Tex tx = make_tex(tile, plan, yccp, B_OFF, g.rot, g.chm);
			const uint32_t yw[2] = {(g.chm & 7u) ? ywrg : 0u,
				((g.chm & 7u) ? (ywba & 0xFFFFu) : 0u) | ((g.chm & 8u) ? (ywba & 0xFFFF0000u) : 0u)};
			// sum over the fit's texels of sum_c p_c^2 (the constant part of its error): word 11 of the fit-geometry cache
			// when every active lane of the wave finds its fit's column there (the starts trip's test), a row loop otherwise
			uint32_t pp_sum = 0;
			const uint32_t gsrc = geo_src(g, kf, wl, lay32);
			const bool ghit = gbase[gsrc + 12*CF_WG_THREADS] == geo_tag(g, id, kf) && (!lay32 || ((gsrc ^ wl) & 32u) == 0u);
			const bool pphit = __ballot(act && !ghit) == 0ull;
			if (pphit)
				pp_sum = gbase[gsrc + 11*CF_WG_THREADS];
			else if constexpr (UNITW) {
				// (with the search's bias taken off, as fit_lane leaves it in the cache: a whole-block fit's from the table word,
				// a partition fit's from its own channel sums)
				uint32_t ssum = 0;
#pragma unroll 1
				for (uint32_t r = 0; r < 4u; ++r) {
					uint32_t P[4];
					planes<true>(tx, *reinterpret_cast<const uint4*>(tx.pl() + 4u*r), P);
					const uint32_t m4 = bytemask4((g.mask >> (4u*r)) & 15u);
#pragma unroll
					for (int c = 0; c < 4; ++c) {
						pp_sum += __builtin_amdgcn_udot4(P[c] & m4, P[c], 0u, false);
						ssum = __builtin_amdgcn_udot4(P[c] & m4, 0x01010101u, ssum, false);
					}
				}
				const uint32_t bias = g.ns < 2u ? lohi_rawsum(lohi[B_OFF >> 2])
					: search_bias_part(ssum, 0u, 0u, 0u, (uint32_t)__builtin_popcount(g.mask), !(g.chm & 8u));
				pp_sum = search_pp_fold(pp_sum, bias);
			} else
				pp_sum = ycc_pp_sum(tx, g.mask, yw);
			// the 4-entry selector search when no active lane's fit has more than 4 palette entries (wave-uniform)
			const bool narrow = __ballot(act && (g.m6 || g.ib > 2u)) == 0ull;
			CF_DIAG_COUNT(CF_DIAG_PERTURB, !(CF_BC7_ABLATE & 32) && (kk == ntop ? uber2 : uber) != 0u);
			CF_DIAG_COUNT(CF_DIAG_PERTURB_NARROW, !(CF_BC7_ABLATE & 32) && (kk == ntop ? uber2 : uber) != 0u && narrow);
#if CF_BC7_DIAG
			const bool nopb = __ballot(act && g.pbk != 0u) == 0ull;   // (a ballot of the whole wave: outside the counter's lane test)
			CF_DIAG_COUNT(CF_DIAG_PERTURB_NOPB, !(CF_BC7_ABLATE & 32) && (kk == ntop ? uber2 : uber) != 0u && nopb);
#endif
			CF_DIAG_COUNT(CF_DIAG_PERTURB_PPHIT, !(CF_BC7_ABLATE & 32) && (kk == ntop ? uber2 : uber) != 0u && pphit);
			const uint32_t S = g.pbk ? 1u : 0u;
			const uint32_t fq0 = g.planes45 ? (g.sca ? 4u : 0u) : 2u*kf, fq1 = fq0 + 1u;   // column words of the fit's fields
#pragma unroll 1
			for (uint32_t r = 0; r < ((CF_BC7_ABLATE & 32) ? 0u : (kk == ntop ? uber2 : uber)); ++r) {
				bool moved = false;
#pragma unroll 1
				for (uint32_t set = 0; set < 2u; ++set) {
					if (!((msets >> set) & 1u))
						continue;
					const uint32_t q0 = wc[fq0*CF_WG_THREADS], q1 = wc[fq1*CF_WG_THREADS];
					const uint32_t pbv = g.planes45 ? 0u : (wc[6*CF_WG_THREADS] >> (2u*kf)) & 3u;
					const uint32_t cur_err = wc[(15u + kf)*CF_WG_THREADS];
					bool valid = act;
					uint32_t nq0 = q0, nq1 = q1, npb = pbv;
					if (set == 0u) {
						const uint32_t e = mv >> 3, ch = (mv >> 1) & 3u, up = mv & 1u;
						const uint32_t bits_c = ch < 3u ? g.cb : g.ab;
						if (bits_c) {
							const uint32_t src = e ? q1 : q0;
							const int nv = (int)((src >> (8u*ch)) & 255u) + (up ? 1 : -1);
							valid = valid && nv >= 0 && nv <= (int)((1u << bits_c) - 1u);
							const uint32_t nw = (src & ~(255u << (8u*ch))) | (((uint32_t)nv & 255u) << (8u*ch));
							nq0 = e ? q0 : nw;
							nq1 = e ? nw : q1;
						} else if (g.pbk == 1u && e == 0u)
							npb = pbv ^ (1u << up);
						else if (g.pbk == 2u && e == 0u && up == 0u)
							npb = pbv ^ 3u;
						else
							valid = false;
					} else {
						const uint32_t ch = mv >> 2, k4 = mv & 3u;
						const uint32_t bits_c = ch < 3u ? g.cb : g.ab;
						const int d0 = (k4 == 0u || k4 == 2u) ? 1 : -1, d1 = (k4 == 0u || k4 == 3u) ? 1 : -1;
						const int v0 = (int)((q0 >> (8u*ch)) & 255u) + d0, v1 = (int)((q1 >> (8u*ch)) & 255u) + d1;
						const int qm = (int)((1u << bits_c) - 1u);
						valid = valid && bits_c != 0u && v0 >= 0 && v0 <= qm && v1 >= 0 && v1 <= qm;
						nq0 = (q0 & ~(255u << (8u*ch))) | (((uint32_t)v0 & 255u) << (8u*ch));
						nq1 = (q1 & ~(255u << (8u*ch))) | (((uint32_t)v1 & 255u) << (8u*ch));
					}
					LaneFit f;
					f.q0 = nq0; f.q1 = nq1; f.pb = npb; f.err = 0;
					// (a move out of the field's range leaves a byte of 255 or 2^bits in nq0 / nq1, which the shift by S pushes into
					// the neighbouring byte: such a lane is not `valid`, its key never wins and its endpoints are not stored)
					const uint32_t tc = g.cb ? g.cb + S : 0u, ta = g.ab ? g.ab + S : 0u;
					const uint32_t fe0 = dequant_word(code_word(nq0, S, npb & S), tc, ta);
					const uint32_t fe1 = dequant_word(code_word(nq1, S, (npb >> 1) & S), tc, ta);
#pragma unroll
					for (int j = 0; j < 4; ++j) f.w[j] = 0;
					float x0[4], x1[4], hq[3];
					bool okk;
					uint32_t arow[4];
					arow_load<UNITW>(tx.tile_, tx.boff, arow);   // (the whole wave is on here)
					if (narrow)
						assign_lsq_lane<UNITW, 4, WIDE ? 4 : 3>(tx, g.mask, g.m6, L_HL & 1u, g.ib, yw, pp_sum, false, fe0, fe1, arow, f, x0, x1, hq, okk);
					else
						assign_lsq_lane<UNITW, 8, WIDE ? 4 : 3>(tx, g.mask, g.m6, L_HL & 1u, g.ib, yw, pp_sum, false, fe0, fe1, arow, f, x0, x1, hq, okk);
					const uint32_t key = valid ? ((f.err << 4) | mv) : 0xFFFFFFFFu;
					uint32_t fitmin = cf_row_min_u32(key);
					if (g.m6) {
						const uint32_t other = (uint32_t)cf_bperm((int)fitmin, lane ^ 16u);
						fitmin = other < fitmin ? other : fitmin;
					}
					const bool win = valid && key == fitmin && f.err < cur_err && (!g.m6 || (L_HL & 1u) == 0u);
					// every fit at once: each puts its own bytes into the weight words of the column; the p-bit word one fit at a time
					if (win)
						column_put_fit(wc, g, kf, nq0, nq1, f.w, f.err);
#pragma unroll 1
					for (uint32_t j = 0; j < 3u; ++j) {
						if (win && !g.planes45 && kf == j)
							column_put_pbits(wc, kf, npb);
						__builtin_amdgcn_wave_barrier();
					}
					moved = moved || __ballot(win) != 0ull;
				}
				if (!moved)
					break;       // no fit of any block of this wave moved: later rounds would repeat this one
			}
			// the owner of the column takes its new total
			CF_FRESH_LANE(lane);
			if (lane == wl && L_CSLOT[18*CF_WG_THREADS] != 0xFFFFFFFFu)
				L_CSLOT[18*CF_WG_THREADS] = L_CSLOT[15*CF_WG_THREADS] + L_CSLOT[16*CF_WG_THREADS] + L_CSLOT[17*CF_WG_THREADS];
			__builtin_amdgcn_wave_barrier();
		}
	}
	CF_FRESH_LANE(lane);
	const uint32_t win_id = cbase[win_lane + 19*CF_WG_THREADS];
	return pack_block_group(cbase + win_lane, win_id, lane, pair);
#undef H_ALPHA
#undef H_GATE
#undef ANY_OPAQUE
#undef TOP_LANE
#undef B_TP
#undef B_OFF
#undef L_H
#undef L_HBASE
#undef L_HL
#undef L_SLOT_OK
#undef L_CSLOT
}

} // namespace

// Waves per SIMD the register allocation is held to.  The kernel is VALU-issue-bound
// (tools/ubench/valu_rate.hip) with LDS / cross-lane latency to hide, and a fourth wave hides 3 %
// more of it (profiles/r02_occupancy_ab.txt).  Round 2 stayed at 3 waves (166 registers) because
// the 128-register build spilled 12 values whose scratch traffic reached HBM (108 MB per launch
// against 84 MB algorithmic).  Round 3 removed what was spilled -- every one a function of the lane
// id or of the wave index: the wave index is a scalar now (loop counter, block index and pair flag
// live in SGPRs), the lane id is re-read with a volatile mbcnt pair where a phase starts, the lane
// roles are expressions of it instead of variables carried through the fit, and __shfl's hidden
// lane-id arithmetic is gone (cf_bperm), and a block's three LDS pointers are one word offset (Tex) --
// so every linear-metric build fits 128 registers with private_segment_fixed_size 0.  Round 5 (second pass of the
// 32-lane layout, gate and ranking state): the perceptual builds take 142 / 146 registers and run at 3 waves
// (held to 128 the 32-lane one spilled one value, 8 B of scratch per lane).
#ifndef CF_BC7_WAVES
#define CF_BC7_WAVES(UNITW, WIDE) ((UNITW) ? 4 : 3)
#endif
template <int PIX, bool UNITW, bool WIDE, int LEVEL>
__global__ void __launch_bounds__(CF_WG_THREADS)
__attribute__((amdgpu_waves_per_eu(CF_BC7_WAVES(UNITW, WIDE), CF_BC7_WAVES(UNITW, WIDE))))
cfhip_bc7_encode_kernel(cf_kparams kp)
{
	__shared__ uint32_t cands[CF_BC7_CAND_WORDS*CF_WG_THREADS];
	__shared__ uint32_t geoc[CF_BC7_GEO_WORDS*CF_WG_THREADS];
	__shared__ __attribute__((aligned(16))) uint32_t tile[CF_BLOCKS_PER_WG*16];
	__shared__ __attribute__((aligned(16))) uint32_t plan[CF_BLOCKS_PER_WG*16];
	__shared__ uint4 outb[CF_BLOCKS_PER_WG];
	__shared__ uint32_t mom[CF_BLOCKS_PER_WG*CF_BC7_MOM_WORDS];
	__shared__ __attribute__((aligned(16))) uint32_t yccp[UNITW ? 4 : CF_BLOCKS_PER_WG*32];
	uint32_t gx_, gy_;
	cf_resolve(kp, gx_, gy_);
	const uint32_t bx0 = gx_*CF_BLOCKS_PER_WG;
	const uint32_t byy = gy_;
	cf_load_tile_rgba8<PIX>(kp, bx0, byy, tile);
	__syncthreads();
	if (!UNITW) {
		// perceptual metric: every texel once as (Y | Cr << 16, Cb | A << 16)
		const uint32_t t = threadIdx.x, p = tile[t];
		uint32_t prg, pba;
		ycc_pairs(p & 255u, (p >> 8) & 255u, (p >> 16) & 255u, p >> 24, prg, pba);
		yccp[2u*t] = prg;
		yccp[2u*t + 1u] = pba;
	}
	{
		// channel-planar copy: plan[b*16 + r*4 + c] = channel c of the 4 texels of row r
		const uint32_t t = threadIdx.x, c = t & 3u;
		const uint4 row = *reinterpret_cast<const uint4*>(tile + (t & ~3u));
		const uint32_t pw = ((row.x >> (8u*c)) & 255u) | (((row.y >> (8u*c)) & 255u) << 8) |
			(((row.z >> (8u*c)) & 255u) << 16) | (((row.w >> (8u*c)) & 255u) << 24);
		plan[t] = pw;
		// per-block table of the four channels' extremes, word c = lo | hi << 8 over the block's 16 texels: this thread's row,
		// then the rows of the other three (lanes 4 and 8 away in the DPP row of 16).  It lives in the block's 16 bytes of
		// outb, which are dead until the block's payload is stored there after its search.
		// (read by the 32-lane layouts' first stream trip)
		// Unit weights: the upper half of every word of the table holds the sum of the block's 64 raw bytes, alpha included
		// whatever the block's channel set (bc7_packed.h: lohi_pack; the bias of a whole-block fit's selector search).  The
		// wide layout has no table of extremes and keeps the sum in word 0 of the block's four.
		uint32_t rs = 0;
		if constexpr (UNITW)
			rs = cf_row_sum_u32(__builtin_amdgcn_udot4(pw, 0x01010101u, 0u, false));   // (a DPP row of 16 lanes = the block's 16 planar words)
		if (!WIDE) {
			const uint32_t lh = byte_lohi(pw);
			uint32_t lo = lh & 255u, hi = lh >> 8, o;
			o = cf_dpp<0x128>(lo); lo = o < lo ? o : lo;   // row_ror:8
			o = cf_dpp<0x128>(hi); hi = o > hi ? o : hi;
			o = cf_dpp<0x124>(lo); lo = o < lo ? o : lo;   // row_ror:4
			o = cf_dpp<0x124>(hi); hi = o > hi ? o : hi;
			if ((t & 12u) == 0u)
				reinterpret_cast<uint32_t*>(outb)[(t >> 4)*4u + c] = UNITW ? lohi_pack(lo | (hi << 8), rs) : lo | (hi << 8);
		} else if constexpr (UNITW) {
			if ((t & 15u) == 0u)
				reinterpret_cast<uint32_t*>(outb)[(t >> 4)*4u] = lohi_pack(0u, rs);
		}
	}
	__syncthreads();
	block_moments_put(plan, mom, threadIdx.x);
	__syncthreads();

	// wave index as a scalar (the loop counter, block index and pair flag then live in SGPRs), lane id
	// from mbcnt where it is needed: nothing derived from threadIdx stays in a VGPR across the phases
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	// the wave's 4 blocks; up to High two neighbouring blocks share one pass
	for (uint32_t j = 0; j < 4u;) {
		const uint32_t b = wave*4u + j;
		if (bx0 + b >= kp.bx)
			break;
		const bool pair = !WIDE && j < 3u && bx0 + b + 1u < kp.bx &&
			!(CF_BC7_ABLATE & 4);
		// opaque copy: keeps the (many) lane-role values of encode_blocks from being hoisted
		// out of this loop and held in registers across all phases
		const uint4 blk = encode_blocks<UNITW, WIDE, LEVEL>(tile, plan, yccp, mom, reinterpret_cast<const uint32_t*>(outb), b, pair, cands + wave*64u, geoc + wave*64u, kp);
		uint32_t lo;
		asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lo));
		if (pair) {
			if ((lo & 31u) == 0u)
				outb[b + (lo >> 5)] = blk;
		} else if (lo == 0u)
			outb[b] = blk;
		j += pair ? 2u : 1u;
	}
	__syncthreads();
	// coalesced payload store: 16 blocks x 16 B = 256 B contiguous
	if (wave == 0u) {
		uint32_t t;
		asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(t));
		const uint32_t b = t >> 2;
		if (bx0 + b < kp.bx) {
			const uint32_t* o = reinterpret_cast<const uint32_t*>(outb);
			uint32_t* dst = reinterpret_cast<uint32_t*>(kp.out +
				((size_t)byy*kp.bx + bx0)*16u);
			dst[t] = o[t];
		}
	}
}

extern "C" hipError_t cfhip_launch_bc7(const cf_kparams* kp, int pixel_type, int unit_weights,
	hipStream_t stream)
{
	dim3 grid((kp->bx + CF_BLOCKS_PER_WG - 1)/CF_BLOCKS_PER_WG, kp->by, 1);
	if (kp->batch)
		grid = dim3(kp->total_wg, 1, 1);
	dim3 block(CF_WG_THREADS, 1, 1);
	// one instance per quality level (levels above Highest run Highest's, like the oracle's clamp)
#define CF_BC7_LAUNCH(P, U, E, L) \
	hipLaunchKernelGGL((cfhip_bc7_encode_kernel<P, U, E, L>), grid, block, 0, stream, *kp)
#define CF_BC7_LEVELS(P, U) \
	switch (kp->quality) { \
		case 0u: CF_BC7_LAUNCH(P, U, false, 0); break; \
		case 1u: CF_BC7_LAUNCH(P, U, false, 1); break; \
		case 2u: CF_BC7_LAUNCH(P, U, false, 2); break; \
		case 3u: CF_BC7_LAUNCH(P, U, true, 3); break; \
		default: CF_BC7_LAUNCH(P, U, true, 4); break; \
	}
	if (pixel_type == 0) {
		if (unit_weights) CF_BC7_LEVELS(0, true) else CF_BC7_LEVELS(0, false)
	} else {
		if (unit_weights) CF_BC7_LEVELS(1, true) else CF_BC7_LEVELS(1, false)
	}
#undef CF_BC7_LEVELS
#undef CF_BC7_LAUNCH
	return hipGetLastError();
}

#if CF_BC7_DIAG
// copy the diagnostic counters to out[0 .. CF_DIAG_N - 1] and zero them
extern "C" hipError_t cfhip_bc7_diag(unsigned long long* out)
{
	hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(cf_bc7_diag), sizeof(cf_bc7_diag));
	const unsigned long long z[CF_DIAG_N] = {};
	if (e == hipSuccess)
		e = hipMemcpyToSymbol(HIP_SYMBOL(cf_bc7_diag), z, sizeof(z));
	return e;
}
#endif
