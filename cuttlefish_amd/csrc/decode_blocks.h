// decode_blocks.h -- the per-format block decoders shared by the decode kernels (decode.hip) and the quality
// metrics (compare.hip): tables, bit helpers, decode4x4<FMT, TYPE> for the 4x4 formats and the ASTC parse into
// an LDS record plus its per-texel evaluation.  Everything lies in an anonymous namespace, so each translation
// unit that includes it gets its own copy of the __constant__ tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---------------------------------------------------------------- tables (public specifications)

__constant__ uint16_t dk_part2[64] = {
	0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80,
	0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000,
	0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310, 0x3100, 0x8cce,
	0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c,
	0xaaaa, 0xf0f0, 0x5a5a, 0x33cc, 0x3c3c, 0x55aa, 0x9696, 0xa55a,
	0x73ce, 0x13c8, 0x324c, 0x3bdc, 0x6996, 0xc33c, 0x9966, 0x0660,
	0x0272, 0x04e4, 0x4e40, 0x2720, 0xc936, 0x936c, 0x39c6, 0x639c,
	0x9336, 0x9cc6, 0x817e, 0xe718, 0xccf0, 0x0fcc, 0x7744, 0xee22};
__constant__ uint32_t dk_part3[64] = {
	0xaa685050, 0x6a5a5040, 0x5a5a4200, 0x5450a0a8, 0xa5a50000, 0xa0a05050, 0x5555a0a0, 0x5a5a5050,
	0xaa550000, 0xaa555500, 0xaaaa5500, 0x90909090, 0x94949494, 0xa4a4a4a4, 0xa9a59450, 0x2a0a4250,
	0xa5945040, 0x0a425054, 0xa5a5a500, 0x55a0a0a0, 0xa8a85454, 0x6a6a4040, 0xa4a45000, 0x1a1a0500,
	0x0050a4a4, 0xaaa59090, 0x14696914, 0x69691400, 0xa08585a0, 0xaa821414, 0x50a4a450, 0x6a5a0200,
	0xa9a58000, 0x5090a0a8, 0xa8a09050, 0x24242424, 0x00aa5500, 0x24924924, 0x24499224, 0x50a50a50,
	0x500aa550, 0xaaaa4444, 0x66660000, 0xa5a0a5a0, 0x50a050a0, 0x69286928, 0x44aaaa44, 0x66666600,
	0xaa444444, 0x54a854a8, 0x95809580, 0x96969600, 0xa85454a8, 0x80959580, 0xaa141414, 0x96960000,
	0xaaaa1414, 0xa05050a0, 0xa0a5a5a0, 0x96000000, 0x40804080, 0xa9a8a9a8, 0xaaaaaa44, 0x2a4a5254};
__constant__ uint8_t dk_anchor2[64] = {
	15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
	15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
	15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6,
	6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15};
__constant__ uint8_t dk_anchor3a[64] = {
	3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3,
	3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
	8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15,
	3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3};
__constant__ uint8_t dk_anchor3b[64] = {
	15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8,
	15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
	15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8,
	15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8};
// interpolation weights of 2-, 3- and 4-bit indices at [0..3], [4..11], [12..27]
__constant__ uint8_t dk_w[28] = {0, 21, 43, 64, 0, 9, 18, 27, 37, 46, 55, 64,
	0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64};
__constant__ int16_t dk_etc_mod[8][2] = {{2, 8}, {5, 17}, {9, 29}, {13, 42}, {18, 60}, {24, 80}, {33, 106}, {47, 183}};
__constant__ uint8_t dk_etc_dist[8] = {3, 6, 11, 16, 23, 32, 41, 64};
__constant__ int8_t dk_eac_mod[16][8] = {
	{-3, -6, -9, -15, 2, 5, 8, 14}, {-3, -7, -10, -13, 2, 6, 9, 12},
	{-2, -5, -8, -13, 1, 4, 7, 12}, {-2, -4, -6, -13, 1, 3, 5, 12},
	{-3, -6, -8, -12, 2, 5, 7, 11}, {-3, -7, -9, -11, 2, 6, 8, 10},
	{-4, -7, -8, -11, 3, 6, 7, 10}, {-3, -5, -8, -11, 2, 4, 7, 10},
	{-2, -6, -8, -10, 1, 5, 7, 9}, {-2, -5, -8, -10, 1, 4, 7, 9},
	{-2, -4, -8, -10, 1, 3, 7, 9}, {-2, -5, -7, -10, 1, 4, 6, 9},
	{-3, -4, -7, -10, 2, 3, 6, 9}, {-1, -2, -3, -10, 0, 1, 2, 9},
	{-4, -6, -8, -9, 3, 5, 7, 8}, {-3, -5, -7, -9, 2, 4, 6, 8}};

// ---------------------------------------------------------------- small helpers

// n (0..32) bits of the 128-bit block at pos; bits at or beyond 128 read as 0
__device__ __forceinline__ uint32_t bits128(uint64_t lo, uint64_t hi, int pos, int n)
{
	if (n <= 0 || pos >= 128)
		return 0u;
	uint64_t v;
	if (pos >= 64)
		v = hi >> (pos - 64);
	else if (pos == 0)
		v = lo;
	else
		v = (lo >> pos) | (hi << (64 - pos));
	return n >= 32 ? (uint32_t)v : (uint32_t)v & ((1u << n) - 1u);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint32_t rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a)
{
	return (r & 255u) | ((g & 255u) << 8) | ((b & 255u) << 16) | (a << 24);
}

__device__ __forceinline__ uint32_t pick4(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t i)
{
	return (i & 2u) ? ((i & 1u) ? p3 : p2) : ((i & 1u) ? p1 : p0);
}

// float -> half, round to nearest even (the oracle's cfo_float_to_half)
__device__ __forceinline__ uint32_t f2h(float f)
{
	const uint32_t x = __float_as_uint(f);
	const uint32_t sign = (x >> 16) & 0x8000u, em = x & 0x7FFFFFFFu;
	if (em >= 0x7F800000u)
		return sign | 0x7C00u | (em > 0x7F800000u ? 0x200u | ((em >> 13) & 0x3FFu) : 0u);
	if (em >= 0x477FF000u)
		return sign | 0x7C00u;
	if (em < 0x33000001u)
		return sign;
	const int e = (int)(em >> 23) - 127;
	const uint32_t m = (em & 0x7FFFFFu) | 0x800000u;
	const int shift = e < -14 ? 13 + (-14 - e) : 13;
	uint32_t hm = m >> shift;
	const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
	if (rem > half || (rem == half && (hm & 1u)))
		++hm;
	const uint32_t he = e < -14 ? 0u : (uint32_t)(e + 15) << 10;
	return (sign | (e < -14 ? hm : (he + hm - 0x400u))) & 0xFFFFu;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

// ---------------------------------------------------------------- per-format block decoders
// Each writes the block's texels as 32-bit words, texel (i, j) at byte i*TB of row j's TB words.

template <int TB>
__device__ __forceinline__ void put8(uint32_t* w, int i, int j, uint32_t v)      // TB = 1
{
	w[j] |= (v & 255u) << (8*i);
}

template <int TB>
__device__ __forceinline__ void put16(uint32_t* w, int i, int j, uint32_t v)     // TB = 2
{
	w[2*j + (i >> 1)] |= (v & 0xFFFFu) << (16*(i & 1));
}

// BC1 colour palette (force4: BC2 / BC3 always use four colours)
__device__ __forceinline__ void bc1_block(uint64_t lo, bool force4, uint32_t* w)
{
	const uint32_t c0 = (uint32_t)lo & 0xFFFFu, c1 = (uint32_t)(lo >> 16) & 0xFFFFu;
	uint32_t e0[3], e1[3];
	{
		uint32_t r = (c0 >> 11) & 31, g = (c0 >> 5) & 63, b = c0 & 31;
		e0[0] = (r << 3) | (r >> 2); e0[1] = (g << 2) | (g >> 4); e0[2] = (b << 3) | (b >> 2);
		r = (c1 >> 11) & 31; g = (c1 >> 5) & 63; b = c1 & 31;
		e1[0] = (r << 3) | (r >> 2); e1[1] = (g << 2) | (g >> 4); e1[2] = (b << 3) | (b >> 2);
	}
	const uint32_t p0 = rgba(e0[0], e0[1], e0[2], 255u), p1 = rgba(e1[0], e1[1], e1[2], 255u);
	uint32_t p2, p3;
	if (c0 > c1 || force4) {
		p2 = rgba((2*e0[0] + e1[0])/3, (2*e0[1] + e1[1])/3, (2*e0[2] + e1[2])/3, 255u);
		p3 = rgba((e0[0] + 2*e1[0])/3, (e0[1] + 2*e1[1])/3, (e0[2] + 2*e1[2])/3, 255u);
	} else {
		p2 = rgba((e0[0] + e1[0])/2, (e0[1] + e1[1])/2, (e0[2] + e1[2])/2, 255u);
		p3 = 0u;
	}
	const uint32_t sel = (uint32_t)(lo >> 32);
#pragma unroll
	for (int t = 0; t < 16; ++t)
		w[t] = pick4(p0, p1, p2, p3, (sel >> (2*t)) & 3u);
}

// BC4 unsigned: value of texel t
__device__ __forceinline__ uint32_t bc4u_texel(uint64_t blk, int t)
{
	const uint32_t a0 = (uint32_t)blk & 255u, a1 = (uint32_t)(blk >> 8) & 255u;
	const uint32_t k = (uint32_t)(blk >> (16 + 3*t)) & 7u;
	if (k == 0) return a0;
	if (k == 1) return a1;
	if (a0 > a1)
		return ((8 - k)*a0 + (k - 1)*a1)/7;
	if (k >= 6)
		return k == 6 ? 0u : 255u;
	return ((6 - k)*a0 + (k - 1)*a1)/5;
}

// BC4 signed (D3D rule: -128 reads as -127; interpolation on +128 biased values)
__device__ __forceinline__ int bc4s_texel(uint64_t blk, int t)
{
	int a0 = (int)(int8_t)(blk & 255u), a1 = (int)(int8_t)((blk >> 8) & 255u);
	a0 = a0 < -127 ? -127 : a0;
	a1 = a1 < -127 ? -127 : a1;
	const int u0 = a0 + 128, u1 = a1 + 128;
	const int k = (int)(blk >> (16 + 3*t)) & 7;
	if (k == 0) return a0;
	if (k == 1) return a1;
	if (a0 > a1)
		return ((8 - k)*u0 + (k - 1)*u1)/7 - 128;
	if (k >= 6)
		return k == 6 ? -127 : 127;
	return ((6 - k)*u0 + (k - 1)*u1)/5 - 128;
}

// ---- BC7: one instantiation per mode, every field width a constant
struct bc7_mode_t { int ns, pb, rb, isb, cb, ab, pbits, ib, ib2; };
constexpr bc7_mode_t kBc7[8] = {
	{3, 4, 0, 0, 4, 0, 1, 3, 0}, {2, 6, 0, 0, 6, 0, 2, 3, 0}, {3, 6, 0, 0, 5, 0, 0, 2, 0},
	{2, 6, 0, 0, 7, 0, 1, 2, 0}, {1, 0, 2, 1, 5, 6, 0, 2, 3}, {1, 0, 2, 0, 7, 8, 0, 2, 2},
	{1, 0, 0, 0, 7, 7, 1, 4, 0}, {2, 6, 0, 0, 5, 5, 1, 2, 0}};

__device__ __forceinline__ uint32_t bc7_weight(int bits, uint32_t idx)
{
	return dk_w[(bits == 2 ? 0 : (bits == 3 ? 4 : 12)) + idx];
}

template <int MODE>
__device__ __forceinline__ void bc7_block(uint64_t lo, uint64_t hi, uint32_t* w)
{
	constexpr bc7_mode_t m = kBc7[MODE];
	constexpr int ne = 2*m.ns;
	int pos = MODE + 1;
	const uint32_t part = bits128(lo, hi, pos, m.pb); pos += m.pb;
	const uint32_t rot = bits128(lo, hi, pos, m.rb); pos += m.rb;
	const uint32_t isel = bits128(lo, hi, pos, m.isb); pos += m.isb;
	uint32_t ep[6][4];
#pragma unroll
	for (int c = 0; c < 3; ++c)
#pragma unroll
		for (int e = 0; e < ne; ++e) {
			ep[e][c] = bits128(lo, hi, pos, m.cb);
			pos += m.cb;
		}
#pragma unroll
	for (int e = 0; e < ne; ++e) {
		ep[e][3] = m.ab ? bits128(lo, hi, pos, m.ab) : 255u;
		pos += m.ab;
	}
	constexpr int cbits = m.cb + (m.pbits ? 1 : 0), abits = m.ab ? m.ab + (m.pbits ? 1 : 0) : 0;
	if (m.pbits) {
		uint32_t pb[6];
#pragma unroll
		for (int e = 0; e < ne; ++e) {
			if (m.pbits == 1 || (e & 1) == 0) {
				pb[e] = bits128(lo, hi, pos, 1);
				pos += 1;
			} else
				pb[e] = pb[e - 1];
		}
#pragma unroll
		for (int e = 0; e < ne; ++e) {
#pragma unroll
			for (int c = 0; c < 3; ++c)
				ep[e][c] = (ep[e][c] << 1) | pb[e];
			if (abits)
				ep[e][3] = (ep[e][3] << 1) | pb[e];
		}
	}
	// the endpoints as RGBA8 words, held in named registers: a select between loads of an array would become
	// an indexed load from a stack array
	auto pack = [&](int e) -> uint32_t {
		uint32_t v[4];
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const uint32_t x = ep[e][c] << (8 - cbits);
			v[c] = (x | (x >> cbits)) & 255u;
		}
		if (abits) {
			const uint32_t x = ep[e][3] << (8 - abits);
			v[3] = (x | (x >> abits)) & 255u;
		} else
			v[3] = ep[e][3];
		return rgba(v[0], v[1], v[2], v[3]);
	};
	const uint32_t P0 = pack(0), P1 = pack(1), P2 = ne > 2 ? pack(2) : 0u, P3 = ne > 2 ? pack(3) : 0u;
	const uint32_t P4 = ne > 4 ? pack(4) : 0u, P5 = ne > 4 ? pack(5) : 0u;
	const uint32_t p2 = m.ns == 2 ? dk_part2[part] : 0u, p3 = m.ns == 3 ? dk_part3[part] : 0u;
	const int a1 = m.ns == 2 ? dk_anchor2[part] : (m.ns == 3 ? dk_anchor3a[part] : 0);
	const int a2 = m.ns == 3 ? dk_anchor3b[part] : 0;
	int pos2 = pos + 16*m.ib - m.ns;        // secondary indices follow the primary ones
#pragma unroll
	for (int i = 0; i < 16; ++i) {
		const uint32_t s = m.ns == 1 ? 0u : (m.ns == 2 ? (p2 >> i) & 1u : (p3 >> (2*i)) & 3u);
		const bool anchor = (s == 0u && i == 0) || (s == 1u && i == a1) || (s == 2u && i == a2);
		const int n = m.ib - (anchor ? 1 : 0);
		const uint32_t idx = bits128(lo, hi, pos, n);
		pos += n;
		uint32_t idx2 = 0;
		if (m.ib2) {
			const int n2 = m.ib2 - (i == 0 ? 1 : 0);
			idx2 = bits128(lo, hi, pos2, n2);
			pos2 += n2;
		}
		uint32_t cw, aw;
		if (m.ib2) {
			if (isel) { cw = bc7_weight(m.ib2, idx2); aw = bc7_weight(m.ib, idx); }
			else { cw = bc7_weight(m.ib, idx); aw = bc7_weight(m.ib2, idx2); }
		} else
			cw = aw = bc7_weight(m.ib, idx);
		const uint32_t e0 = s == 0u ? P0 : (s == 1u ? P2 : P4);
		const uint32_t e1 = s == 0u ? P1 : (s == 1u ? P3 : P5);
		uint32_t px[4];
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			const uint32_t x0 = (e0 >> (8*c)) & 255u, x1 = (e1 >> (8*c)) & 255u, ww = c < 3 ? cw : aw;
			px[c] = ((64 - ww)*x0 + ww*x1 + 32) >> 6;
		}
		if (m.rb) {
			const uint32_t a = px[3];
			if (rot == 1) { px[3] = px[0]; px[0] = a; }
			else if (rot == 2) { px[3] = px[1]; px[1] = a; }
			else if (rot == 3) { px[3] = px[2]; px[2] = a; }
		}
		w[i] = rgba(px[0], px[1], px[2], px[3]);
	}
}

__device__ __forceinline__ void bc7_decode(uint64_t lo, uint64_t hi, uint32_t* w)
{
	const uint32_t b0 = (uint32_t)lo & 255u;
	switch (b0 ? __builtin_ctz(b0) : 8) {
		case 0: bc7_block<0>(lo, hi, w); break;
		case 1: bc7_block<1>(lo, hi, w); break;
		case 2: bc7_block<2>(lo, hi, w); break;
		case 3: bc7_block<3>(lo, hi, w); break;
		case 4: bc7_block<4>(lo, hi, w); break;
		case 5: bc7_block<5>(lo, hi, w); break;
		case 6: bc7_block<6>(lo, hi, w); break;
		case 7: bc7_block<7>(lo, hi, w); break;
		default:
#pragma unroll
			for (int i = 0; i < 16; ++i)
				w[i] = 0u;
			break;
	}
}

// ---- BC6H: the 14 mode layouts as runs of payload bits (oracle/bc6h_decode.c), one instantiation per mode
enum { F_RW, F_RX, F_RY, F_RZ, F_GW, F_GX, F_GY, F_GZ, F_BW, F_BX, F_BY, F_BZ, F_D, F_N };
struct bc6_run { int start, field, lo, count; };
struct bc6_mode_t { int mode_bits, mode_val, two, transformed, ebits, dr, dg, db; bc6_run runs[24]; };
#define R_(s, f, lo, n) {s, f, lo, n}
constexpr bc6_mode_t kBc6[14] = {
	{2, 0x00, 1, 1, 10, 5, 5, 5, {R_(2, F_GY, 4, 1), R_(3, F_BY, 4, 1), R_(4, F_BZ, 4, 1),
		R_(5, F_RW, 0, 10), R_(15, F_GW, 0, 10), R_(25, F_BW, 0, 10), R_(35, F_RX, 0, 5),
		R_(40, F_GZ, 4, 1), R_(41, F_GY, 0, 4), R_(45, F_GX, 0, 5), R_(50, F_BZ, 0, 1),
		R_(51, F_GZ, 0, 4), R_(55, F_BX, 0, 5), R_(60, F_BZ, 1, 1), R_(61, F_BY, 0, 4),
		R_(65, F_RY, 0, 5), R_(70, F_BZ, 2, 1), R_(71, F_RZ, 0, 5), R_(76, F_BZ, 3, 1),
		R_(77, F_D, 0, 5)}},
	{2, 0x01, 1, 1, 7, 6, 6, 6, {R_(2, F_GY, 5, 1), R_(3, F_GZ, 4, 1), R_(4, F_GZ, 5, 1),
		R_(5, F_RW, 0, 7), R_(12, F_BZ, 0, 1), R_(13, F_BZ, 1, 1), R_(14, F_BY, 4, 1),
		R_(15, F_GW, 0, 7), R_(22, F_BY, 5, 1), R_(23, F_BZ, 2, 1), R_(24, F_GY, 4, 1),
		R_(25, F_BW, 0, 7), R_(32, F_BZ, 3, 1), R_(33, F_BZ, 5, 1), R_(34, F_BZ, 4, 1),
		R_(35, F_RX, 0, 6), R_(41, F_GY, 0, 4), R_(45, F_GX, 0, 6), R_(51, F_GZ, 0, 4),
		R_(55, F_BX, 0, 6), R_(61, F_BY, 0, 4), R_(65, F_RY, 0, 6), R_(71, F_RZ, 0, 6),
		R_(77, F_D, 0, 5)}},
	{5, 0x02, 1, 1, 11, 5, 4, 4, {R_(5, F_RW, 0, 10), R_(15, F_GW, 0, 10), R_(25, F_BW, 0, 10),
		R_(35, F_RX, 0, 5), R_(40, F_RW, 10, 1), R_(41, F_GY, 0, 4), R_(45, F_GX, 0, 4),
		R_(49, F_GW, 10, 1), R_(50, F_BZ, 0, 1), R_(51, F_GZ, 0, 4), R_(55, F_BX, 0, 4),
		R_(59, F_BW, 10, 1), R_(60, F_BZ, 1, 1), R_(61, F_BY, 0, 4), R_(65, F_RY, 0, 5),
		R_(70, F_BZ, 2, 1), R_(71, F_RZ, 0, 5), R_(76, F_BZ, 3, 1), R_(77, F_D, 0, 5)}},
	{5, 0x06, 1, 1, 11, 4, 5, 4, {R_(5, F_RW, 0, 10), R_(15, F_GW, 0, 10), R_(25, F_BW, 0, 10),
		R_(35, F_RX, 0, 4), R_(39, F_RW, 10, 1), R_(40, F_GZ, 4, 1), R_(41, F_GY, 0, 4),
		R_(45, F_GX, 0, 5), R_(50, F_GW, 10, 1), R_(51, F_GZ, 0, 4), R_(55, F_BX, 0, 4),
		R_(59, F_BW, 10, 1), R_(60, F_BZ, 1, 1), R_(61, F_BY, 0, 4), R_(65, F_RY, 0, 4),
		R_(69, F_BZ, 0, 1), R_(70, F_BZ, 2, 1), R_(71, F_RZ, 0, 4), R_(75, F_GY, 4, 1),
		R_(76, F_BZ, 3, 1), R_(77, F_D, 0, 5)}},
	{5, 0x0A, 1, 1, 11, 4, 4, 5, {R_(5, F_RW, 0, 10), R_(15, F_GW, 0, 10), R_(25, F_BW, 0, 10),
		R_(35, F_RX, 0, 4), R_(39, F_RW, 10, 1), R_(40, F_BY, 4, 1), R_(41, F_GY, 0, 4),
		R_(45, F_GX, 0, 4), R_(49, F_GW, 10, 1), R_(50, F_BZ, 0, 1), R_(51, F_GZ, 0, 4),
		R_(55, F_BX, 0, 5), R_(60, F_BW, 10, 1), R_(61, F_BY, 0, 4), R_(65, F_RY, 0, 4),
		R_(69, F_BZ, 1, 1), R_(70, F_BZ, 2, 1), R_(71, F_RZ, 0, 4), R_(75, F_BZ, 4, 1),
		R_(76, F_BZ, 3, 1), R_(77, F_D, 0, 5)}},
	{5, 0x0E, 1, 1, 9, 5, 5, 5, {R_(5, F_RW, 0, 9), R_(14, F_BY, 4, 1), R_(15, F_GW, 0, 9),
		R_(24, F_GY, 4, 1), R_(25, F_BW, 0, 9), R_(34, F_BZ, 4, 1), R_(35, F_RX, 0, 5),
		R_(40, F_GZ, 4, 1), R_(41, F_GY, 0, 4), R_(45, F_GX, 0, 5), R_(50, F_BZ, 0, 1),
		R_(51, F_GZ, 0, 4), R_(55, F_BX, 0, 5), R_(60, F_BZ, 1, 1), R_(61, F_BY, 0, 4),
		R_(65, F_RY, 0, 5), R_(70, F_BZ, 2, 1), R_(71, F_RZ, 0, 5), R_(76, F_BZ, 3, 1),
		R_(77, F_D, 0, 5)}},
	{5, 0x12, 1, 1, 8, 6, 5, 5, {R_(5, F_RW, 0, 8), R_(13, F_GZ, 4, 1), R_(14, F_BY, 4, 1),
		R_(15, F_GW, 0, 8), R_(23, F_BZ, 2, 1), R_(24, F_GY, 4, 1), R_(25, F_BW, 0, 8),
		R_(33, F_BZ, 3, 1), R_(34, F_BZ, 4, 1), R_(35, F_RX, 0, 6), R_(41, F_GY, 0, 4),
		R_(45, F_GX, 0, 5), R_(50, F_BZ, 0, 1), R_(51, F_GZ, 0, 4), R_(55, F_BX, 0, 5),
		R_(60, F_BZ, 1, 1), R_(61, F_BY, 0, 4), R_(65, F_RY, 0, 6), R_(71, F_RZ, 0, 6),
		R_(77, F_D, 0, 5)}},
	{5, 0x16, 1, 1, 8, 5, 6, 5, {R_(5, F_RW, 0, 8), R_(13, F_BZ, 0, 1), R_(14, F_BY, 4, 1),
		R_(15, F_GW, 0, 8), R_(23, F_GY, 5, 1), R_(24, F_GY, 4, 1), R_(25, F_BW, 0, 8),
		R_(33, F_GZ, 5, 1), R_(34, F_BZ, 4, 1), R_(35, F_RX, 0, 5), R_(40, F_GZ, 4, 1),
		R_(41, F_GY, 0, 4), R_(45, F_GX, 0, 6), R_(51, F_GZ, 0, 4), R_(55, F_BX, 0, 5),
		R_(60, F_BZ, 1, 1), R_(61, F_BY, 0, 4), R_(65, F_RY, 0, 5), R_(70, F_BZ, 2, 1),
		R_(71, F_RZ, 0, 5), R_(76, F_BZ, 3, 1), R_(77, F_D, 0, 5)}},
	{5, 0x1A, 1, 1, 8, 5, 5, 6, {R_(5, F_RW, 0, 8), R_(13, F_BZ, 1, 1), R_(14, F_BY, 4, 1),
		R_(15, F_GW, 0, 8), R_(23, F_BY, 5, 1), R_(24, F_GY, 4, 1), R_(25, F_BW, 0, 8),
		R_(33, F_BZ, 5, 1), R_(34, F_BZ, 4, 1), R_(35, F_RX, 0, 5), R_(40, F_GZ, 4, 1),
		R_(41, F_GY, 0, 4), R_(45, F_GX, 0, 5), R_(50, F_BZ, 0, 1), R_(51, F_GZ, 0, 4),
		R_(55, F_BX, 0, 6), R_(61, F_BY, 0, 4), R_(65, F_RY, 0, 5), R_(70, F_BZ, 2, 1),
		R_(71, F_RZ, 0, 5), R_(76, F_BZ, 3, 1), R_(77, F_D, 0, 5)}},
	{5, 0x1E, 1, 0, 6, 6, 6, 6, {R_(5, F_RW, 0, 6), R_(11, F_GZ, 4, 1), R_(12, F_BZ, 0, 1),
		R_(13, F_BZ, 1, 1), R_(14, F_BY, 4, 1), R_(15, F_GW, 0, 6), R_(21, F_GY, 5, 1),
		R_(22, F_BY, 5, 1), R_(23, F_BZ, 2, 1), R_(24, F_GY, 4, 1), R_(25, F_BW, 0, 6),
		R_(31, F_GZ, 5, 1), R_(32, F_BZ, 3, 1), R_(33, F_BZ, 5, 1), R_(34, F_BZ, 4, 1),
		R_(35, F_RX, 0, 6), R_(41, F_GY, 0, 4), R_(45, F_GX, 0, 6), R_(51, F_GZ, 0, 4),
		R_(55, F_BX, 0, 6), R_(61, F_BY, 0, 4), R_(65, F_RY, 0, 6), R_(71, F_RZ, 0, 6),
		R_(77, F_D, 0, 5)}},
	{5, 0x03, 0, 0, 10, 10, 10, 10, {R_(5, F_RW, 0, 10), R_(15, F_GW, 0, 10), R_(25, F_BW, 0, 10),
		R_(35, F_RX, 0, 10), R_(45, F_GX, 0, 10), R_(55, F_BX, 0, 10)}},
	{5, 0x07, 0, 1, 11, 9, 9, 9, {R_(5, F_RW, 0, 10), R_(15, F_GW, 0, 10), R_(25, F_BW, 0, 10),
		R_(35, F_RX, 0, 9), R_(44, F_RW, 10, 1), R_(45, F_GX, 0, 9), R_(54, F_GW, 10, 1),
		R_(55, F_BX, 0, 9), R_(64, F_BW, 10, 1)}},
	{5, 0x0B, 0, 1, 12, 8, 8, 8, {R_(5, F_RW, 0, 10), R_(15, F_GW, 0, 10), R_(25, F_BW, 0, 10),
		R_(35, F_RX, 0, 8), R_(43, F_RW, 11, -2), R_(45, F_GX, 0, 8), R_(53, F_GW, 11, -2),
		R_(55, F_BX, 0, 8), R_(63, F_BW, 11, -2)}},
	{5, 0x0F, 0, 1, 16, 4, 4, 4, {R_(5, F_RW, 0, 10), R_(15, F_GW, 0, 10), R_(25, F_BW, 0, 10),
		R_(35, F_RX, 0, 4), R_(39, F_RW, 15, -6), R_(45, F_GX, 0, 4), R_(49, F_GW, 15, -6),
		R_(55, F_BX, 0, 4), R_(59, F_BW, 15, -6)}},
};
#undef R_

__device__ __forceinline__ int sext(int v, int bits)
{
	const int m = 1 << (bits - 1);
	return (v ^ m) - m;
}

__device__ __forceinline__ int bc6_unq(int q, int bits, bool sgn)
{
	if (!sgn) {
		if (bits >= 15) return q;
		if (q == 0) return 0;
		if (q == (1 << bits) - 1) return 0xFFFF;
		return ((q << 16) + 0x8000) >> bits;
	}
	if (bits >= 16) return q;
	int s = 0, u;
	if (q < 0) { s = 1; q = -q; }
	if (q == 0) u = 0;
	else if (q >= (1 << (bits - 1)) - 1) u = 0x7FFF;
	else u = ((q << 15) + 0x4000) >> (bits - 1);
	return s ? -u : u;
}

__device__ __forceinline__ uint32_t bc6_fin(int v, bool sgn)
{
	if (!sgn) return (uint32_t)((v*31) >> 6) & 0xFFFFu;
	if (v < 0) return (0x8000u | (uint32_t)(((-v)*31) >> 5)) & 0xFFFFu;
	return (uint32_t)((v*31) >> 5) & 0xFFFFu;
}

template <int MODE, bool SGN>
__device__ __forceinline__ void bc6_block(uint64_t lo, uint64_t hi, uint32_t* w)
{
	constexpr bc6_mode_t m = kBc6[MODE];
	int f[F_N];
#pragma unroll
	for (int k = 0; k < F_N; ++k)
		f[k] = 0;
#pragma unroll
	for (int r = 0; r < 24; ++r) {
		if (m.runs[r].count == 0)
			continue;
		const int n = m.runs[r].count < 0 ? -m.runs[r].count : m.runs[r].count;
		const uint32_t v = bits128(lo, hi, m.runs[r].start, n);
#pragma unroll
		for (int i = 0; i < 16; ++i)
			if (i < n) {
				const int fb = m.runs[r].count < 0 ? m.runs[r].lo - i : m.runs[r].lo + i;
				f[m.runs[r].field] |= (int)((v >> i) & 1u) << fb;
			}
	}
	int e[4][3] = {{f[F_RW], f[F_GW], f[F_BW]}, {f[F_RX], f[F_GX], f[F_BX]},
		{f[F_RY], f[F_GY], f[F_BY]}, {f[F_RZ], f[F_GZ], f[F_BZ]}};
	constexpr int dbits[3] = {m.dr, m.dg, m.db};
	constexpr int ne = m.two ? 4 : 2;
	if (SGN)
#pragma unroll
		for (int c = 0; c < 3; ++c)
			e[0][c] = sext(e[0][c], m.ebits);
	if (m.transformed) {
#pragma unroll
		for (int k = 1; k < ne; ++k)
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				const int d = sext(e[k][c], dbits[c]);
				const int v = (e[0][c] + d) & ((1 << m.ebits) - 1);
				e[k][c] = SGN ? sext(v, m.ebits) : v;
			}
	} else if (SGN) {
#pragma unroll
		for (int k = 1; k < ne; ++k)
#pragma unroll
			for (int c = 0; c < 3; ++c)
				e[k][c] = sext(e[k][c], dbits[c]);
	}
#pragma unroll
	for (int k = 0; k < ne; ++k)
#pragma unroll
		for (int c = 0; c < 3; ++c)
			e[k][c] = bc6_unq(e[k][c], m.ebits, SGN);
	const uint32_t part = m.two ? (uint32_t)f[F_D] : 0u;
	int pos = m.two ? 82 : 65;
	constexpr int ib = m.two ? 3 : 4;
	const uint32_t p2 = m.two ? dk_part2[part] : 0u;
	const int anchor1 = m.two ? dk_anchor2[part] : 0;
#pragma unroll
	for (int i = 0; i < 16; ++i) {
		const uint32_t s = m.two ? (p2 >> i) & 1u : 0u;
		const int nb = ib - ((i == 0 || (s && i == anchor1)) ? 1 : 0);
		const uint32_t idx = bits128(lo, hi, pos, nb);
		pos += nb;
		const int wt = (int)dk_w[(m.two ? 4 : 12) + idx];
		uint32_t h[3];
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const int x0 = s ? e[ne > 2 ? 2 : 0][c] : e[0][c], x1 = s ? e[ne > 2 ? 3 : 1][c] : e[1][c];
			h[c] = bc6_fin(((64 - wt)*x0 + wt*x1 + 32) >> 6, SGN);
		}
		w[2*i] = h[0] | (h[1] << 16);
		w[2*i + 1] = h[2] | (0x3C00u << 16);
	}
}

template <bool SGN>
__device__ __forceinline__ bool bc6_decode(uint64_t lo, uint64_t hi, uint32_t* w)
{
	const uint32_t mv2 = (uint32_t)lo & 3u, mv5 = (uint32_t)lo & 31u;
	int mode = -1;
	if (mv2 < 2) mode = (int)mv2;
	else
		switch (mv5) {
			case 0x02: mode = 2; break; case 0x06: mode = 3; break; case 0x0A: mode = 4; break;
			case 0x0E: mode = 5; break; case 0x12: mode = 6; break; case 0x16: mode = 7; break;
			case 0x1A: mode = 8; break; case 0x1E: mode = 9; break; case 0x03: mode = 10; break;
			case 0x07: mode = 11; break; case 0x0B: mode = 12; break; case 0x0F: mode = 13; break;
			default: break;
		}
	switch (mode) {
		case 0: bc6_block<0, SGN>(lo, hi, w); return true;
		case 1: bc6_block<1, SGN>(lo, hi, w); return true;
		case 2: bc6_block<2, SGN>(lo, hi, w); return true;
		case 3: bc6_block<3, SGN>(lo, hi, w); return true;
		case 4: bc6_block<4, SGN>(lo, hi, w); return true;
		case 5: bc6_block<5, SGN>(lo, hi, w); return true;
		case 6: bc6_block<6, SGN>(lo, hi, w); return true;
		case 7: bc6_block<7, SGN>(lo, hi, w); return true;
		case 8: bc6_block<8, SGN>(lo, hi, w); return true;
		case 9: bc6_block<9, SGN>(lo, hi, w); return true;
		case 10: bc6_block<10, SGN>(lo, hi, w); return true;
		case 11: bc6_block<11, SGN>(lo, hi, w); return true;
		case 12: bc6_block<12, SGN>(lo, hi, w); return true;
		case 13: bc6_block<13, SGN>(lo, hi, w); return true;
		default:
			// reserved modes decode to zero RGB (the oracle's rule), alpha 1.0 like every BC6H texel
#pragma unroll
			for (int i = 0; i < 16; ++i) {
				w[2*i] = 0u;
				w[2*i + 1] = 0x3C00u << 16;
			}
			return false;
	}
}

// ---- ETC1 / ETC2 RGB (blk: the 8 colour bytes as loaded, little-endian)
__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
__device__ __forceinline__ int ex4(int v) { return (v << 4) | v; }
__device__ __forceinline__ int ex5(int v) { return (v << 3) | (v >> 2); }
__device__ __forceinline__ int ex6(int v) { return (v << 2) | (v >> 4); }
__device__ __forceinline__ int ex7(int v) { return (v << 1) | (v >> 6); }
__device__ __forceinline__ int sx3(int v) { return v >= 4 ? v - 8 : v; }

// texels of the RGB part, row-major RGBA8 (alpha 255, or 0 for the punch-through texels of RGBA1)
__device__ __forceinline__ void etc_rgb_block(uint64_t blk, bool a1, uint32_t* w)
{
	const uint32_t hi = bswap32((uint32_t)blk), lo = bswap32((uint32_t)(blk >> 32));
	int diff = (hi >> 1) & 1;
	const int flip = hi & 1;
	const int opaque = a1 ? diff : 1;
	if (a1)
		diff = 1;
	int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0}, mode = 0;   // 0 individual/differential, 1 T, 2 H, 3 planar
	if (!diff) {
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			b0[c] = ex4((hi >> (28 - 8*c)) & 15);
			b1[c] = ex4((hi >> (24 - 8*c)) & 15);
		}
	} else {
		int q[3], d[3];
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			q[c] = (hi >> (27 - 8*c)) & 31;
			d[c] = sx3((hi >> (24 - 8*c)) & 7);
		}
		if (q[0] + d[0] < 0 || q[0] + d[0] > 31) mode = 1;
		else if (q[1] + d[1] < 0 || q[1] + d[1] > 31) mode = 2;
		else if (q[2] + d[2] < 0 || q[2] + d[2] > 31) mode = 3;
		else
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				b0[c] = ex5(q[c]);
				b1[c] = ex5(q[c] + d[c]);
			}
	}
	// T / H: the four paint colours; planar: O, H, V
	uint32_t paint[4] = {0u, 0u, 0u, 0u};
	int O[3] = {0, 0, 0}, Hc[3] = {0, 0, 0}, V[3] = {0, 0, 0};
	if (mode == 1) {
		int c1[3], c2[3];
		c1[0] = ex4((int)(((hi >> 27) & 3) << 2 | ((hi >> 24) & 3)));
		c1[1] = ex4((hi >> 20) & 15); c1[2] = ex4((hi >> 16) & 15);
		c2[0] = ex4((hi >> 12) & 15); c2[1] = ex4((hi >> 8) & 15); c2[2] = ex4((hi >> 4) & 15);
		const int d = dk_etc_dist[((hi >> 2) & 3) << 1 | (hi & 1)];
		paint[0] = rgba(c1[0], c1[1], c1[2], 255u);
		paint[1] = rgba(clamp255(c2[0] + d), clamp255(c2[1] + d), clamp255(c2[2] + d), 255u);
		paint[2] = rgba(c2[0], c2[1], c2[2], 255u);
		paint[3] = rgba(clamp255(c2[0] - d), clamp255(c2[1] - d), clamp255(c2[2] - d), 255u);
	} else if (mode == 2) {
		const int r1 = (hi >> 27) & 15, g1 = (int)(((hi >> 24) & 7) << 1 | ((hi >> 20) & 1));
		const int bb1 = (int)(((hi >> 19) & 1) << 3 | ((hi >> 15) & 7));
		const int r2 = (hi >> 11) & 15, g2 = (hi >> 7) & 15, bb2 = (hi >> 3) & 15;
		const int w1 = (r1 << 8) | (g1 << 4) | bb1, w2 = (r2 << 8) | (g2 << 4) | bb2;
		const int d = dk_etc_dist[(int)(((hi >> 2) & 1) << 2 | (hi & 1) << 1) | (w1 >= w2 ? 1 : 0)];
		const int c1[3] = {ex4(r1), ex4(g1), ex4(bb1)}, c2[3] = {ex4(r2), ex4(g2), ex4(bb2)};
		paint[0] = rgba(clamp255(c1[0] + d), clamp255(c1[1] + d), clamp255(c1[2] + d), 255u);
		paint[1] = rgba(clamp255(c1[0] - d), clamp255(c1[1] - d), clamp255(c1[2] - d), 255u);
		paint[2] = rgba(clamp255(c2[0] + d), clamp255(c2[1] + d), clamp255(c2[2] + d), 255u);
		paint[3] = rgba(clamp255(c2[0] - d), clamp255(c2[1] - d), clamp255(c2[2] - d), 255u);
	} else if (mode == 3) {
		// planar: each clamped channel is pinned to a register before packing.  With the clamp folded into
		// the packing, gfx950 returned 255 for some in-range blue values at x = 3 of random planar blocks.
		O[0] = ex6((hi >> 25) & 63);
		O[1] = ex7((int)(((hi >> 24) & 1) << 6 | ((hi >> 17) & 63)));
		O[2] = ex6((int)(((hi >> 16) & 1) << 5 | ((hi >> 11) & 3) << 3 | ((hi >> 7) & 7)));
		Hc[0] = ex6((int)(((hi >> 2) & 31) << 1 | (hi & 1)));
		Hc[1] = ex7((lo >> 25) & 127);
		Hc[2] = ex6((lo >> 19) & 63);
		V[0] = ex6((lo >> 13) & 63);
		V[1] = ex7((lo >> 6) & 127);
		V[2] = ex6(lo & 63);
	}
	const int t0 = (hi >> 5) & 7, t1 = (hi >> 2) & 7;
	const int ma0 = dk_etc_mod[t0][0], mb0 = dk_etc_mod[t0][1], ma1 = dk_etc_mod[t1][0], mb1 = dk_etc_mod[t1][1];
#pragma unroll
	for (int x = 0; x < 4; ++x)
#pragma unroll
		for (int y = 0; y < 4; ++y) {
			const int k = x*4 + y;
			const uint32_t v = ((lo >> (16 + k)) & 1u) << 1 | ((lo >> k) & 1u);
			uint32_t o;
			if (!opaque && v == 2u && mode != 3)     // punch-through (not in the planar mode)
				o = 0u;
			else if (mode == 0) {
				const int sub = flip ? (y >= 2) : (x >= 2);
				int a = sub ? ma1 : ma0;
				const int b = sub ? mb1 : mb0;
				if (!opaque)
					a = 0;
				const int m = v == 0u ? a : (v == 1u ? b : (v == 2u ? -a : -b));
				o = rgba(clamp255((sub ? b1[0] : b0[0]) + m), clamp255((sub ? b1[1] : b0[1]) + m),
					clamp255((sub ? b1[2] : b0[2]) + m), 255u);
			} else if (mode == 3) {
				int pc[3];
#pragma unroll
				for (int c = 0; c < 3; ++c) {
					pc[c] = clamp255((x*(Hc[c] - O[c]) + y*(V[c] - O[c]) + 4*O[c] + 2) >> 2);
					asm volatile("" : "+v"(pc[c]));    // see the note at the planar colours above
				}
				o = rgba(pc[0], pc[1], pc[2], 255u);
			} else
				o = pick4(paint[0], paint[1], paint[2], paint[3], v);
			w[y*4 + x] = o;
		}
}

// EAC: value of texel (x, y); kind 0 alpha8, 1 R11 unsigned, 2 R11 signed
__device__ __forceinline__ int eac_texel(uint64_t blk, int kind, int x, int y)
{
	int base = kind == 2 ? (int)(int8_t)(blk & 255u) : (int)(blk & 255u);
	const int b1 = (int)(blk >> 8) & 255;
	const int mult = b1 >> 4, table = b1 & 15;
	if (kind == 2 && base == -128)
		base = -127;
	// bytes 2..7 big-endian
	const uint64_t bits = __builtin_bswap64(blk) & 0xFFFFFFFFFFFFull;
	const int k = x*4 + y;
	const int idx = (int)((bits >> (45 - 3*k)) & 7u);
	const int m = dk_eac_mod[table][idx];
	if (kind == 0)
		return clamp255(base + m*mult);
	if (kind == 1)
		return clampi(base*8 + 4 + (mult ? m*mult*8 : m), 0, 2047);
	return clampi(base*8 + (mult ? m*mult*8 : m), -1023, 1023);
}

// texel bytes of a 4x4 format's decoded layout
template <int FMT, int TYPE>
constexpr int texel_bytes()
{
	return FMT == 33 ? 1 : (FMT == 34 ? 2 : (FMT == 41 ? 2 : (FMT == 42 ? 4 : (FMT == 35 ? 8 : 4))));
}

// decode one block into w (4*TB words); returns true for an error block
template <int FMT, int TYPE>
__device__ __forceinline__ bool decode4x4(uint64_t lo, uint64_t hi, uint32_t* w)
{
	constexpr int TB = texel_bytes<FMT, TYPE>();
#pragma unroll
	for (int k = 0; k < 4*TB; ++k)
		w[k] = 0u;
	if constexpr (FMT == 29 || FMT == 30) {
		bc1_block(lo, false, w);
	} else if constexpr (FMT == 31) {
		bc1_block(hi, true, w);
#pragma unroll
		for (int i = 0; i < 16; ++i)
			w[i] = (w[i] & 0xFFFFFFu) | ((uint32_t)((lo >> (4*i)) & 15u)*17u << 24);
	} else if constexpr (FMT == 32) {
		bc1_block(hi, true, w);
#pragma unroll
		for (int i = 0; i < 16; ++i)
			w[i] = (w[i] & 0xFFFFFFu) | (bc4u_texel(lo, i) << 24);
	} else if constexpr (FMT == 33 || FMT == 34) {
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			const uint32_t r = TYPE == 1 ? (uint32_t)bc4s_texel(lo, i) & 255u : bc4u_texel(lo, i);
			if constexpr (FMT == 33)
				put8<1>(w, i & 3, i >> 2, r);
			else {
				const uint32_t g = TYPE == 1 ? (uint32_t)bc4s_texel(hi, i) & 255u : bc4u_texel(hi, i);
				put16<2>(w, i & 3, i >> 2, r | (g << 8));
			}
		}
	} else if constexpr (FMT == 35) {
		return !bc6_decode<TYPE == 5>(lo, hi, w);
	} else if constexpr (FMT == 36) {
		bc7_decode(lo, hi, w);
	} else if constexpr (FMT >= 37 && FMT <= 39) {
		etc_rgb_block(lo, FMT == 39, w);
	} else if constexpr (FMT == 40) {
		etc_rgb_block(hi, false, w);
#pragma unroll
		for (int y = 0; y < 4; ++y)
#pragma unroll
			for (int x = 0; x < 4; ++x)
				w[y*4 + x] = (w[y*4 + x] & 0xFFFFFFu) | ((uint32_t)eac_texel(lo, 0, x, y) << 24);
	} else if constexpr (FMT == 41 || FMT == 42) {
		const int kind = TYPE == 1 ? 2 : 1;
#pragma unroll
		for (int y = 0; y < 4; ++y)
#pragma unroll
			for (int x = 0; x < 4; ++x) {
				const uint32_t r = (uint32_t)eac_texel(lo, kind, x, y) & 0xFFFFu;
				if constexpr (FMT == 41)
					put16<2>(w, x, y, r);
				else
					w[y*4 + x] = r | (((uint32_t)eac_texel(hi, kind, x, y) & 0xFFFFu) << 16);
			}
	}
	return false;
}

__device__ __forceinline__ void load_block(const uint8_t* p, int bytes, bool vec, uint64_t& lo, uint64_t& hi)
{
	if (vec) {
		if (bytes == 16) {
			const uint4 v = *reinterpret_cast<const uint4*>(p);
			lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
			hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
		} else {
			const uint2 v = *reinterpret_cast<const uint2*>(p);
			lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
			hi = 0;
		}
		return;
	}
	lo = hi = 0;
	for (int i = 0; i < bytes; ++i) {
		const uint64_t b = p[i];
		if (i < 8) lo |= b << (8*i);
		else hi |= b << (8*(i - 8));
	}
}

// ---------------------------------------------------------------- ASTC

struct AstcQ { uint8_t bits, trits, quints; };
// weight ranges 0..11 and colour ranges 0..16 (levels 2 .. 32, 6 .. 256)
__constant__ AstcQ dk_wq[12] = {{1, 0, 0}, {0, 1, 0}, {2, 0, 0}, {0, 0, 1}, {1, 1, 0}, {3, 0, 0},
	{1, 0, 1}, {2, 1, 0}, {4, 0, 0}, {2, 0, 1}, {3, 1, 0}, {5, 0, 0}};
__constant__ AstcQ dk_cq[17] = {{1, 1, 0}, {3, 0, 0}, {1, 0, 1}, {2, 1, 0}, {4, 0, 0}, {2, 0, 1},
	{3, 1, 0}, {5, 0, 0}, {3, 0, 1}, {4, 1, 0}, {6, 0, 0}, {4, 0, 1}, {5, 1, 0}, {7, 0, 0},
	{5, 0, 1}, {6, 1, 0}, {8, 0, 0}};

__device__ __forceinline__ int ise_bits(int count, AstcQ q)
{
	return count*q.bits + (q.trits ? (8*count + 4)/5 : 0) + (q.quints ? (7*count + 2)/3 : 0);
}

__device__ __forceinline__ int weight_unq(AstcQ q, int v)
{
	const int m = v & ((1 << q.bits) - 1), d = v >> q.bits;
	int r;
	if (!q.trits && !q.quints) {
		switch (q.bits) {
			case 1: r = m ? 63 : 0; break;
			case 2: r = (m << 4) | (m << 2) | m; break;
			case 3: r = (m << 3) | m; break;
			case 4: r = (m << 2) | (m >> 2); break;
			default: r = (m << 1) | (m >> 4); break;
		}
	} else if (q.bits == 0) {
		if (q.trits) r = d == 0 ? 0 : (d == 1 ? 32 : 63);
		else r = d == 0 ? 0 : (d == 1 ? 16 : (d == 2 ? 32 : (d == 3 ? 47 : 63)));
	} else {
		const int a = (m & 1) ? 0x7F : 0, b = (m >> 1) & 1, c = (m >> 2) & 1;
		int B, C;
		if (q.trits) {
			if (q.bits == 1) { B = 0; C = 50; }
			else if (q.bits == 2) { B = (b << 6) | (b << 2) | b; C = 23; }
			else { B = (c << 6) | (b << 5) | (c << 1) | b; C = 11; }
		} else {
			if (q.bits == 1) { B = 0; C = 28; }
			else { B = (b << 6) | (b << 1); C = 13; }
		}
		int T = d*C + B;
		T ^= a;
		r = (a & 0x20) | (T >> 2);
	}
	return r > 32 ? r + 1 : r;
}

__device__ __forceinline__ int color_unq(AstcQ q, int v)
{
	const int n = q.bits, m = v & ((1 << n) - 1), d = v >> n;
	if (!q.trits && !q.quints) {
		int r = 0, have = 0;
		while (have < 8) {
			r = (r << n) | m;
			have += n;
		}
		return (r >> (have - 8)) & 255;
	}
	const int A = (m & 1) ? 0x1FF : 0;
	const int b = (m >> 1) & 1, c = (m >> 2) & 1, dd = (m >> 3) & 1, e = (m >> 4) & 1, f = (m >> 5) & 1;
	int B = 0, C = 0;
	if (q.trits) {
		switch (n) {
			case 1: B = 0; C = 204; break;
			case 2: B = (b << 8) | (b << 4) | (b << 2) | (b << 1); C = 93; break;
			case 3: B = (c << 8) | (b << 7) | (c << 3) | (b << 2) | (c << 1) | b; C = 44; break;
			case 4: B = (dd << 8) | (c << 7) | (b << 6) | (dd << 2) | (c << 1) | b; C = 22; break;
			case 5: B = (e << 8) | (dd << 7) | (c << 6) | (b << 5) | (e << 1) | dd; C = 11; break;
			default: B = (f << 8) | (e << 7) | (dd << 6) | (c << 5) | (b << 4) | f; C = 5; break;
		}
	} else {
		switch (n) {
			case 1: B = 0; C = 113; break;
			case 2: B = (b << 8) | (b << 3) | (b << 2); C = 54; break;
			case 3: B = (c << 8) | (b << 7) | (c << 2) | (b << 1) | c; C = 26; break;
			case 4: B = (dd << 8) | (c << 7) | (b << 6) | (dd << 1) | c; C = 13; break;
			default: B = (e << 8) | (dd << 7) | (c << 6) | (b << 5) | e; C = 6; break;
		}
	}
	int T = d*C + B;
	T ^= A;
	return (A & 0x80) | (T >> 2);
}

// trit k (0..4) of a packed 8-bit T
__device__ __forceinline__ int trit_of(int T, int k)
{
	int t4, t3, C;
	if (((T >> 2) & 7) == 7) {
		C = (((T >> 5) & 7) << 2) | (T & 3);
		t4 = 2; t3 = 2;
	} else {
		C = T & 0x1F;
		if (((T >> 5) & 3) == 3) { t4 = 2; t3 = (T >> 7) & 1; }
		else { t4 = (T >> 7) & 1; t3 = (T >> 5) & 3; }
	}
	int t2, t1, t0;
	if ((C & 3) == 3) {
		t2 = 2; t1 = (C >> 4) & 1;
		t0 = (((C >> 3) & 1) << 1) | (((C >> 2) & 1) & ~((C >> 3) & 1));
	} else if (((C >> 2) & 3) == 3) {
		t2 = 2; t1 = 2; t0 = C & 3;
	} else {
		t2 = (C >> 4) & 1; t1 = (C >> 2) & 3;
		t0 = (((C >> 1) & 1) << 1) | ((C & 1) & ~((C >> 1) & 1));
	}
	return k == 0 ? t0 : (k == 1 ? t1 : (k == 2 ? t2 : (k == 3 ? t3 : t4)));
}

__device__ __forceinline__ int quint_of(int Q, int k)
{
	int q0, q1, q2;
	if (((Q >> 1) & 3) == 3 && ((Q >> 5) & 3) == 0) {
		const int b = Q & 1;
		q2 = (b << 2) | ((((Q >> 4) & 1) & ~b) << 1) | (((Q >> 3) & 1) & ~b);
		q1 = 4; q0 = 4;
	} else {
		int C;
		if (((Q >> 1) & 3) == 3) {
			q2 = 4;
			C = (((Q >> 3) & 3) << 3) | ((~(Q >> 5) & 3) << 1) | (Q & 1);
		} else {
			q2 = (Q >> 5) & 3;
			C = Q & 0x1F;
		}
		if ((C & 7) == 5) { q1 = 4; q0 = (C >> 3) & 3; }
		else { q1 = (C >> 3) & 3; q0 = C & 7; }
	}
	return k == 0 ? q0 : (k == 1 ? q1 : q2);
}

// integer sequence decode of `count` values from bit `pos` of (lo, hi) into LDS
__device__ __forceinline__ void ise_decode(AstcQ q, uint64_t lo, uint64_t hi, int pos, int count, uint8_t* vals)
{
	const int n = q.bits, end = pos + ise_bits(count, q);
	if (q.trits) {
		for (int i = 0; i < count; i += 5) {
			int m[5] = {0, 0, 0, 0, 0}, T = 0;
#pragma unroll
			for (int k = 0; k < 5; ++k)
				if (i + k < count) {
					constexpr int tb[5] = {2, 2, 1, 2, 1}, ts[5] = {0, 2, 4, 5, 7};
					m[k] = (int)bits128(lo, hi, pos, n);
					pos += n;
					int nb = tb[k];
					if (pos + nb > end) nb = end - pos;
					T |= (int)bits128(lo, hi, pos, nb) << ts[k];
					pos += nb;
				}
#pragma unroll
			for (int k = 0; k < 5; ++k)
				if (i + k < count)
					vals[i + k] = (uint8_t)((trit_of(T, k) << n) | m[k]);
		}
	} else if (q.quints) {
		for (int i = 0; i < count; i += 3) {
			int m[3] = {0, 0, 0}, Q = 0;
#pragma unroll
			for (int k = 0; k < 3; ++k)
				if (i + k < count) {
					constexpr int qb[3] = {3, 2, 2}, qs[3] = {0, 3, 5};
					m[k] = (int)bits128(lo, hi, pos, n);
					pos += n;
					int nb = qb[k];
					if (pos + nb > end) nb = end - pos;
					Q |= (int)bits128(lo, hi, pos, nb) << qs[k];
					pos += nb;
				}
#pragma unroll
			for (int k = 0; k < 3; ++k)
				if (i + k < count)
					vals[i + k] = (uint8_t)((quint_of(Q, k) << n) | m[k]);
		}
	} else {
		for (int i = 0; i < count; ++i, pos += n)
			vals[i] = (uint8_t)bits128(lo, hi, pos, n);
	}
}

__device__ __forceinline__ int parse_block_mode(int mode, int& N, int& M, int& wq, int& dual)
{
	const int R0 = (mode >> 4) & 1, A = (mode >> 5) & 3, B = (mode >> 7) & 3;
	int R1, R2, H = (mode >> 9) & 1, D = (mode >> 10) & 1;
	if (mode & 3) {
		R1 = mode & 1;
		R2 = (mode >> 1) & 1;
		switch ((mode >> 2) & 3) {
			case 0: N = B + 4; M = A + 2; break;
			case 1: N = B + 8; M = A + 2; break;
			case 2: N = A + 2; M = B + 8; break;
			default:
				if (!((mode >> 8) & 1)) { N = A + 2; M = (B & 1) + 6; }
				else { N = (B & 1) + 2; M = A + 2; }
				break;
		}
	} else {
		if (!(mode & 0xC))
			return -1;
		R1 = (mode >> 2) & 1;
		R2 = (mode >> 3) & 1;
		switch (B) {
			case 0: N = 12; M = A + 2; break;
			case 1: N = A + 2; M = 12; break;
			case 2: N = A + 6; M = ((mode >> 9) & 3) + 6; H = 0; D = 0; break;
			default:
				if (A == 0) { N = 6; M = 10; }
				else if (A == 1) { N = 10; M = 6; }
				else return -1;
				break;
		}
	}
	const int r = (R2 << 2) | (R1 << 1) | R0;
	if (r < 2)
		return -1;
	wq = (r - 2) + 6*H;
	dual = D;
	return 0;
}

__device__ __forceinline__ void bit_transfer_signed(int& a, int& b)
{
	b >>= 1;
	b |= a & 0x80;
	a >>= 1;
	a &= 0x3F;
	if (a & 0x20)
		a -= 0x40;
}

__device__ __forceinline__ int c12(int v) { return v < 0 ? 0 : (v > 4095 ? 4095 : v); }

// HDR endpoint mode 7 (base RGB + scale)
__device__ __forceinline__ void hdr_rgb_scale(const int* v, int* e0, int* e1)
{
	const int v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
	const int modeval = ((v0 & 0xC0) >> 6) | (((v1 & 0x80) >> 7) << 2) | (((v2 & 0x80) >> 7) << 3);
	int majcomp, mode;
	if ((modeval & 0xC) != 0xC) { majcomp = modeval >> 2; mode = modeval & 3; }
	else if (modeval != 0xF) { majcomp = modeval & 3; mode = 4; }
	else { majcomp = 0; mode = 5; }
	int red = v0 & 0x3F, green = v1 & 0x1F, blue = v2 & 0x1F, scale = v3 & 0x1F;
	const int bit0 = (v1 >> 6) & 1, bit1 = (v1 >> 5) & 1, bit2 = (v2 >> 6) & 1, bit3 = (v2 >> 5) & 1;
	const int bit4 = (v3 >> 7) & 1, bit5 = (v3 >> 6) & 1, bit6 = (v3 >> 5) & 1;
	const int oh = 1 << mode;
	if (oh & 0x30) green |= bit0 << 6;
	if (oh & 0x3A) green |= bit1 << 5;
	if (oh & 0x30) blue |= bit2 << 6;
	if (oh & 0x3A) blue |= bit3 << 5;
	if (oh & 0x3D) scale |= bit6 << 5;
	if (oh & 0x2D) scale |= bit5 << 6;
	if (oh & 0x04) scale |= bit4 << 7;
	if (oh & 0x3B) red |= bit4 << 6;
	if (oh & 0x04) red |= bit3 << 6;
	if (oh & 0x10) red |= bit5 << 7;
	if (oh & 0x0F) red |= bit2 << 7;
	if (oh & 0x05) red |= bit1 << 8;
	if (oh & 0x0A) red |= bit0 << 8;
	if (oh & 0x05) red |= bit0 << 9;
	if (oh & 0x02) red |= bit6 << 9;
	if (oh & 0x01) red |= bit3 << 10;
	if (oh & 0x02) red |= bit5 << 10;
	const int sh = (0x543211 >> (4*mode)) & 0xF;     // shift amounts 1 1 2 3 4 5
	red <<= sh; green <<= sh; blue <<= sh; scale <<= sh;
	if (mode != 5) { green = red - green; blue = red - blue; }
	int t;
	if (majcomp == 1) { t = red; red = green; green = t; }
	if (majcomp == 2) { t = red; red = blue; blue = t; }
	int r0 = red - scale, g0 = green - scale, b0 = blue - scale;
	red = red < 0 ? 0 : red; green = green < 0 ? 0 : green; blue = blue < 0 ? 0 : blue;
	r0 = r0 < 0 ? 0 : r0; g0 = g0 < 0 ? 0 : g0; b0 = b0 < 0 ? 0 : b0;
	e0[0] = r0 << 4; e0[1] = g0 << 4; e0[2] = b0 << 4; e0[3] = 0x7800;
	e1[0] = red << 4; e1[1] = green << 4; e1[2] = blue << 4; e1[3] = 0x7800;
}

// HDR endpoint mode 11 (and the RGB of 14 / 15)
__device__ __forceinline__ void hdr_rgb(const int* v, int* e0, int* e1)
{
	const int v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5];
	const int majcomp = ((v4 & 0x80) >> 7) | (((v5 & 0x80) >> 7) << 1);
	if (majcomp == 3) {
		e0[0] = v0 << 8; e0[1] = v2 << 8; e0[2] = (v4 & 0x7F) << 9;
		e1[0] = v1 << 8; e1[1] = v3 << 8; e1[2] = (v5 & 0x7F) << 9;
		return;
	}
	const int mode = ((v1 & 0x80) >> 7) | (((v2 & 0x80) >> 7) << 1) | (((v3 & 0x80) >> 7) << 2);
	int a = v0 | ((v1 & 0x40) << 2), b0 = v2 & 0x3F, b1 = v3 & 0x3F, c = v1 & 0x3F;
	int d0 = v4 & 0x7F, d1 = v5 & 0x7F;
	const int dbits = (0x65656767 >> (4*mode)) & 0xF;  // 7 6 7 6 5 6 5 6
	const int bit0 = (v2 >> 6) & 1, bit1 = (v3 >> 6) & 1, bit2 = (v4 >> 6) & 1, bit3 = (v5 >> 6) & 1;
	const int bit4 = (v4 >> 5) & 1, bit5 = (v5 >> 5) & 1;
	const int oh = 1 << mode;
	if (oh & 0xA4) a |= bit0 << 9;
	if (oh & 0x08) a |= bit2 << 9;
	if (oh & 0x50) a |= bit4 << 9;
	if (oh & 0x50) a |= bit5 << 10;
	if (oh & 0xA0) a |= bit1 << 10;
	if (oh & 0xC0) a |= bit2 << 11;
	if (oh & 0x04) c |= bit1 << 6;
	if (oh & 0xE8) c |= bit3 << 6;
	if (oh & 0x20) c |= bit2 << 7;
	if (oh & 0x5B) { b0 |= bit0 << 6; b1 |= bit1 << 6; }
	if (oh & 0x12) { b0 |= bit2 << 7; b1 |= bit3 << 7; }
	d0 &= (1 << dbits) - 1; d1 &= (1 << dbits) - 1;
	if (d0 & (1 << (dbits - 1))) d0 -= 1 << dbits;
	if (d1 & (1 << (dbits - 1))) d1 -= 1 << dbits;
	const int sh = (mode >> 1) ^ 3;
	a <<= sh; b0 <<= sh; b1 <<= sh; c <<= sh; d0 *= 1 << sh; d1 *= 1 << sh;
	int red1 = c12(a), green1 = c12(a - b0), blue1 = c12(a - b1);
	int red0 = c12(a - c), green0 = c12(a - b0 - c - d0), blue0 = c12(a - b1 - c - d1);
	int t;
	if (majcomp == 1) { t = red0; red0 = green0; green0 = t; t = red1; red1 = green1; green1 = t; }
	if (majcomp == 2) { t = red0; red0 = blue0; blue0 = t; t = red1; red1 = blue1; blue1 = t; }
	e0[0] = red0 << 4; e0[1] = green0 << 4; e0[2] = blue0 << 4;
	e1[0] = red1 << 4; e1[1] = green1 << 4; e1[2] = blue1 << 4;
}

__device__ __forceinline__ void hdr_alpha(int v6, int v7, int& a0, int& a1)
{
	const int selector = ((v6 >> 7) & 1) | ((v7 >> 6) & 2);
	v6 &= 0x7F; v7 &= 0x7F;
	if (selector == 3) {
		a0 = v6 << 9; a1 = v7 << 9;
		return;
	}
	v6 |= (v7 << (selector + 1)) & 0x780;
	v7 &= 0x3F >> selector;
	v7 ^= 32 >> selector;
	v7 -= 32 >> selector;
	v6 <<= 4 - selector;
	v7 <<= 4 - selector;
	v7 += v6;
	v7 = v7 < 0 ? 0 : (v7 > 0xFFF ? 0xFFF : v7);
	a0 = v6 << 4; a1 = v7 << 4;
}

// endpoint pair of one partition: 0 LDR, 1 HDR rgb + HDR alpha, 2 HDR rgb + LDR alpha
__device__ __forceinline__ int unpack_endpoints(int cem, const int* v, int* e0, int* e1)
{
	switch (cem) {
		case 0:
			e0[0] = e0[1] = e0[2] = v[0]; e0[3] = 255;
			e1[0] = e1[1] = e1[2] = v[1]; e1[3] = 255;
			return 0;
		case 1: {
			const int L0 = (v[0] >> 2) | (v[1] & 0xC0);
			int L1 = L0 + (v[1] & 0x3F);
			if (L1 > 255) L1 = 255;
			e0[0] = e0[1] = e0[2] = L0; e0[3] = 255;
			e1[0] = e1[1] = e1[2] = L1; e1[3] = 255;
			return 0;
		}
		case 4:
			e0[0] = e0[1] = e0[2] = v[0]; e0[3] = v[2];
			e1[0] = e1[1] = e1[2] = v[1]; e1[3] = v[3];
			return 0;
		case 5: {
			int a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3];
			bit_transfer_signed(a1, a0);
			bit_transfer_signed(a3, a2);
			e0[0] = e0[1] = e0[2] = a0; e0[3] = a2;
			e1[0] = e1[1] = e1[2] = clamp255(a0 + a1); e1[3] = clamp255(a2 + a3);
			return 0;
		}
		case 6:
		case 10:
			e0[0] = (v[0]*v[3]) >> 8; e0[1] = (v[1]*v[3]) >> 8; e0[2] = (v[2]*v[3]) >> 8;
			e1[0] = v[0]; e1[1] = v[1]; e1[2] = v[2];
			e0[3] = cem == 10 ? v[4] : 255;
			e1[3] = cem == 10 ? v[5] : 255;
			return 0;
		case 8:
		case 12: {
			const int s0 = v[0] + v[2] + v[4], s1 = v[1] + v[3] + v[5];
			const int a0 = cem == 12 ? v[6] : 255, a1 = cem == 12 ? v[7] : 255;
			if (s1 >= s0) {
				e0[0] = v[0]; e0[1] = v[2]; e0[2] = v[4]; e0[3] = a0;
				e1[0] = v[1]; e1[1] = v[3]; e1[2] = v[5]; e1[3] = a1;
			} else {
				e0[0] = (v[1] + v[5]) >> 1; e0[1] = (v[3] + v[5]) >> 1; e0[2] = v[5]; e0[3] = a1;
				e1[0] = (v[0] + v[4]) >> 1; e1[1] = (v[2] + v[4]) >> 1; e1[2] = v[4]; e1[3] = a0;
			}
			return 0;
		}
		case 9:
		case 13: {
			int a[8];
#pragma unroll
			for (int i = 0; i < 8; ++i)
				a[i] = (i < 6 || cem == 13) ? v[i] : 0;
			bit_transfer_signed(a[1], a[0]);
			bit_transfer_signed(a[3], a[2]);
			bit_transfer_signed(a[5], a[4]);
			if (cem == 13)
				bit_transfer_signed(a[7], a[6]);
			const int al0 = cem == 13 ? a[6] : 255, al1 = cem == 13 ? a[6] + a[7] : 255;
			int x0[4], x1[4];
			if (a[1] + a[3] + a[5] >= 0) {
				x0[0] = a[0]; x0[1] = a[2]; x0[2] = a[4]; x0[3] = al0;
				x1[0] = a[0] + a[1]; x1[1] = a[2] + a[3]; x1[2] = a[4] + a[5]; x1[3] = al1;
			} else {
				x0[0] = a[0] + a[1]; x0[1] = a[2] + a[3]; x0[2] = a[4] + a[5]; x0[3] = al1;
				x1[0] = a[0]; x1[1] = a[2]; x1[2] = a[4]; x1[3] = al0;
				x0[0] = (x0[0] + x0[2]) >> 1; x0[1] = (x0[1] + x0[2]) >> 1;
				x1[0] = (x1[0] + x1[2]) >> 1; x1[1] = (x1[1] + x1[2]) >> 1;
			}
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				e0[c] = clamp255(x0[c]);
				e1[c] = clamp255(x1[c]);
			}
			return 0;
		}
		case 2: {
			int y0, y1;
			if (v[1] >= v[0]) { y0 = v[0] << 4; y1 = v[1] << 4; }
			else { y0 = (v[1] << 4) + 8; y1 = (v[0] << 4) - 8; }
			e0[0] = e0[1] = e0[2] = y0 << 4; e0[3] = 0x7800;
			e1[0] = e1[1] = e1[2] = y1 << 4; e1[3] = 0x7800;
			return 1;
		}
		case 3: {
			int y0, d;
			if (v[0] & 0x80) { y0 = ((v[1] & 0xE0) << 4) | ((v[0] & 0x7F) << 2); d = (v[1] & 0x1F) << 2; }
			else { y0 = ((v[1] & 0xF0) << 4) | ((v[0] & 0x7F) << 1); d = (v[1] & 0x0F) << 1; }
			const int y1 = y0 + d > 0xFFF ? 0xFFF : y0 + d;
			e0[0] = e0[1] = e0[2] = y0 << 4; e0[3] = 0x7800;
			e1[0] = e1[1] = e1[2] = y1 << 4; e1[3] = 0x7800;
			return 1;
		}
		case 7:
			hdr_rgb_scale(v, e0, e1);
			return 1;
		default:      // 11, 14, 15
			hdr_rgb(v, e0, e1);
			if (cem == 11) { e0[3] = e1[3] = 0x7800; return 1; }
			if (cem == 14) { e0[3] = v[6]; e1[3] = v[7]; return 2; }
			hdr_alpha(v[6], v[7], e0[3], e1[3]);
			return 1;
	}
}

__device__ __forceinline__ uint32_t hash52(uint32_t p)
{
	p ^= p >> 15; p -= p << 17; p += p << 7; p += p << 4;
	p ^= p >> 5; p += p << 16; p ^= p >> 7; p ^= p >> 3;
	p ^= p << 6; p ^= p >> 17;
	return p;
}

__device__ __forceinline__ int select_partition(int seed, int x, int y, int partitions, bool small)
{
	if (partitions <= 1)
		return 0;
	if (small) { x <<= 1; y <<= 1; }
	seed += (partitions - 1)*1024;
	const uint32_t rnum = hash52((uint32_t)seed);
	uint32_t s[8];
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		const uint32_t v = (rnum >> (4*k)) & 0xFu;
		s[k] = (v*v) & 0xFFu;
	}
	int sh1, sh2;
	if (seed & 1) { sh1 = (seed & 2) ? 4 : 5; sh2 = (partitions == 3) ? 6 : 5; }
	else { sh1 = (partitions == 3) ? 6 : 5; sh2 = (seed & 2) ? 4 : 5; }
#pragma unroll
	for (int k = 0; k < 8; ++k)
		s[k] >>= (k & 1) ? sh2 : sh1;
	int a = (int)s[0]*x + (int)s[1]*y + (int)(rnum >> 14);
	int b = (int)s[2]*x + (int)s[3]*y + (int)(rnum >> 10);
	int c = (int)s[4]*x + (int)s[5]*y + (int)(rnum >> 6);
	int d = (int)s[6]*x + (int)s[7]*y + (int)(rnum >> 2);
	a &= 0x3F; b &= 0x3F; c &= 0x3F; d &= 0x3F;
	if (partitions < 4) d = 0;
	if (partitions < 3) c = 0;
	if (a >= b && a >= c && a >= d) return 0;
	if (b >= c && b >= d) return 1;
	if (c >= d) return 2;
	return 3;
}

// LDS record of one parsed block
struct AstcRec {
	uint8_t w[64];            // unquantised grid weights, plane-interleaved as stored
	uint16_t ep[4][2][4];     // endpoint pairs per partition (LDR 0..255, HDR 16-bit LNS)
	uint8_t cv[20];           // colour values of the parse (scratch of phase 1)
	int8_t status;            // 0 normal, 1 void extent (colour in ep[0][0]), -1 error block
	uint8_t kind[4];          // per partition: 0 LDR, 1 HDR, 2 HDR rgb + LDR alpha, 3 HDR under LDR (error colour)
	uint8_t N, M, dual, ccs, parts, ve_hdr, bad;
	uint16_t seed;
};

__device__ __forceinline__ void astc_parse(uint64_t lo, uint64_t hi, int bw, int bh, bool hdr, AstcRec& r)
{
	r.bad = 0;
	const int mode = (int)bits128(lo, hi, 0, 11);
	if ((mode & 0x1FF) == 0x1FC) {
		r.status = -1;
		if (bits128(lo, hi, 10, 2) != 3u)
			return;
		const int isHdr = (mode >> 9) & 1;
		if (isHdr && !hdr)
			return;
		const uint32_t x0 = bits128(lo, hi, 12, 13), x1 = bits128(lo, hi, 25, 13);
		const uint32_t y0 = bits128(lo, hi, 38, 13), y1 = bits128(lo, hi, 51, 13);
		const bool all1 = x0 == 0x1FFFu && x1 == 0x1FFFu && y0 == 0x1FFFu && y1 == 0x1FFFu;
		if (!all1 && (x0 >= x1 || y0 >= y1))
			return;
		for (int c = 0; c < 4; ++c)
			r.ep[0][0][c] = (uint16_t)bits128(lo, hi, 64 + 16*c, 16);
		r.ve_hdr = (uint8_t)isHdr;
		r.status = 1;
		return;
	}
	r.status = -1;
	int N, M, wq, dual;
	if (parse_block_mode(mode, N, M, wq, dual) != 0)
		return;
	const int nw = N*M*(dual ? 2 : 1);
	if (N > bw || M > bh || nw > 64)
		return;
	const AstcQ wqq = dk_wq[wq];
	const int wbits = ise_bits(nw, wqq);
	if (wbits < 24 || wbits > 96)
		return;
	const int parts = (int)bits128(lo, hi, 11, 2) + 1;
	if (dual && parts == 4)
		return;
	int cstart, extra = 0, nvals = 0, seed = 0;
	int cems = 0;                       // 4 bits per partition
	if (parts == 1) {
		cems = (int)bits128(lo, hi, 13, 4);
		cstart = 17;
	} else {
		seed = (int)bits128(lo, hi, 13, 10);
		const uint32_t sel = bits128(lo, hi, 23, 6);
		cstart = 29;
		if ((sel & 3u) == 0u) {
			for (int p = 0; p < parts; ++p)
				cems |= (int)((sel >> 2) & 15u) << (4*p);
		} else {
			extra = 3*parts - 4;
			const uint32_t all = sel | (bits128(lo, hi, 128 - wbits - extra, extra) << 6);
			const int base = (int)(all & 3u) - 1;
			for (int p = 0; p < parts; ++p) {
				const int cls = base + (int)((all >> (2 + p)) & 1u);
				const int m = (int)((all >> (2 + parts + 2*p)) & 3u);
				cems |= ((cls << 2) | m) << (4*p);
			}
		}
	}
	for (int p = 0; p < parts; ++p)
		nvals += 2*(((cems >> (4*p)) >> 2 & 3) + 1);
	if (nvals > 18)
		return;
	const int cbits = 128 - wbits - cstart - extra - (dual ? 2 : 0);
	if (cbits < (13*nvals + 4)/5)
		return;
	int lv = -1;
	for (int q = 0; q < 17; ++q)
		if (ise_bits(nvals, dk_cq[q]) <= (cbits > 128 ? 128 : cbits))
			lv = q;
	if (lv < 0)
		return;
	r.ccs = dual ? (uint8_t)bits128(lo, hi, 128 - wbits - extra - 2, 2) : 0;
	const AstcQ cq = dk_cq[lv];
	ise_decode(cq, lo, hi, cstart, nvals, r.cv);
	int pos = 0;
	for (int p = 0; p < parts; ++p) {
		const int cem = (cems >> (4*p)) & 15;
		const int k = 2*((cem >> 2) + 1);
		int v[8];
#pragma unroll
		for (int i = 0; i < 8; ++i)
			v[i] = i < k ? color_unq(cq, r.cv[pos + i]) : 0;
		pos += k;
		int e0[4], e1[4];
		int kind = unpack_endpoints(cem, v, e0, e1);
		if (!hdr && ((0xC88C >> cem) & 1))    // HDR endpoint modes 2 3 7 11 14 15 under the LDR profile
			kind = 3;
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			r.ep[p][0][c] = (uint16_t)e0[c];
			r.ep[p][1][c] = (uint16_t)e1[c];
		}
		r.kind[p] = (uint8_t)kind;
	}
	// weights: the bit-reversed stream from the top of the block
	const uint64_t rlo = ((uint64_t)__builtin_bitreverse32((uint32_t)(hi >> 32))) |
		((uint64_t)__builtin_bitreverse32((uint32_t)hi) << 32);
	const uint64_t rhi = ((uint64_t)__builtin_bitreverse32((uint32_t)(lo >> 32))) |
		((uint64_t)__builtin_bitreverse32((uint32_t)lo) << 32);
	ise_decode(wqq, rlo, rhi, 0, nw, r.w);
	for (int i = 0; i < nw; ++i)
		r.w[i] = (uint8_t)weight_unq(wqq, r.w[i]);
	r.N = (uint8_t)N; r.M = (uint8_t)M; r.dual = (uint8_t)dual; r.parts = (uint8_t)parts;
	r.seed = (uint16_t)seed;
	r.status = 0;
	// LDR profile: an error block when any texel of the whole footprint (inside the image or not) falls in a
	// partition with HDR endpoints
	int hdr_parts = 0;
	for (int p = 0; p < parts; ++p)
		hdr_parts |= (r.kind[p] == 3) << p;
	if (hdr_parts) {
		const int n = bw*bh;
		for (int i = 0; i < n && !r.bad; ++i)
			if ((hdr_parts >> select_partition(seed, i % bw, i / bw, parts, n < 31)) & 1)
				r.bad = 1;
	}
}

__device__ __forceinline__ uint32_t lns_to_half(int c)
{
	const int e = c >> 11, m = c & 0x7FF;
	int mt;
	if (m < 512) mt = 3*m;
	else if (m < 1536) mt = 4*m - 512;
	else mt = 5*m - 2048;
	const int h = (e << 10) + (mt >> 3);
	return (uint32_t)(h > 0x7BFF ? 0x7BFF : h);
}

// texel (s, t) of a parsed block: RGBA8 (LDR) in out[0], or 4 halves (HDR) in out[0..1]
template <bool HDR>
__device__ __forceinline__ void astc_texel(const AstcRec& r, int bw, int bh, int s, int t, uint32_t* out)
{
	const int n = bw*bh;
	if (r.status < 0) {
		if (HDR) { out[0] = out[1] = 0xFFFFFFFFu; }
		else out[0] = 0xFFFF00FFu;
		return;
	}
	if (r.status == 1) {
		uint32_t h[4];
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			const uint32_t v = r.ep[0][0][c];
			if (!HDR) h[c] = v >> 8;
			else if (r.ve_hdr) h[c] = v;
			else h[c] = f2h((float)v*(1.0f/65535.0f));
		}
		if (HDR) { out[0] = h[0] | (h[1] << 16); out[1] = h[2] | (h[3] << 16); }
		else out[0] = rgba(h[0], h[1], h[2], h[3]);
		return;
	}
	const int p = select_partition(r.seed, s, t, r.parts, n < 31);
	const int kind = r.kind[p];
	if (!HDR && kind == 3) {
		out[0] = 0xFFFF00FFu;
		return;
	}
	// bilinear infill of the N x M grid (specification formulas)
	const int N = r.N, M = r.M, planes = r.dual ? 2 : 1;
	const int Ds = (1024 + bw/2)/(bw - 1), Dt = (1024 + bh/2)/(bh - 1);
	const int gs = (Ds*s*(N - 1) + 32) >> 6, gt = (Dt*t*(M - 1) + 32) >> 6;
	const int js = gs >> 4, fs = gs & 15, jt = gt >> 4, ft = gt & 15;
	const int w11 = (fs*ft + 8) >> 4, w10 = ft - w11, w01 = fs - w11, w00 = 16 - fs - ft + w11;
	const int v0 = js + jt*N;
	int wpl[2];
#pragma unroll
	for (int pl = 0; pl < 2; ++pl) {
		int acc = 8;
		if (pl < planes) {
			acc += w00*r.w[v0*planes + pl];
			if (w01) acc += w01*r.w[(v0 + 1)*planes + pl];
			if (w10) acc += w10*r.w[(v0 + N)*planes + pl];
			if (w11) acc += w11*r.w[(v0 + N + 1)*planes + pl];
		}
		wpl[pl] = acc >> 4;
	}
	uint32_t h[4];
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		const int w = (r.dual && c == r.ccs) ? wpl[1] : wpl[0];
		const int x0 = r.ep[p][0][c], x1 = r.ep[p][1][c];
		if (!HDR) {
			const int C0 = x0*257, C1 = x1*257;
			h[c] = (uint32_t)(((C0*(64 - w) + C1*w + 32) >> 6) >> 8);
		} else {
			const bool isHdr = kind == 1 || (kind == 2 && c < 3);
			const int C0 = isHdr ? x0 : x0*257, C1 = isHdr ? x1 : x1*257;
			const int C = (C0*(64 - w) + C1*w + 32) >> 6;
			if (isHdr) h[c] = lns_to_half(C);
			else h[c] = C == 65535 ? 0x3C00u : f2h((float)C*(1.0f/65536.0f));
		}
	}
	if (HDR) { out[0] = h[0] | (h[1] << 16); out[1] = h[2] | (h[3] << 16); }
	else out[0] = rgba(h[0], h[1], h[2], h[3]);
}

} // namespace
