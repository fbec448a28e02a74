// BC7 endpoint arithmetic on whole code words (bytes r,g,b,a) instead of one channel at a time.
// Plain integer functions: the kernels of bc7_encode.hip use them on the device, a host program can
// include this file and compare them with the per-byte formulas (tests/test_bc7_packed_identities.py).
// Every identity here is exact, so the encoder's payloads do not depend on which form computes them.
// Below them: the integer moments of a set of texels as packed words (the block table, what phase 1 hands to the fits),
// compared with per-texel sums by tests/test_bc7_moment_derivation.py.
#ifndef CFHIP_BC7_PACKED_H
#define CFHIP_BC7_PACKED_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CF_PK __host__ __device__ __forceinline__
#else
#define CF_PK static inline
#endif
// product of two operands that fit 24 bits: the device has a full-rate instruction for it
#if defined(__HIP_DEVICE_COMPILE__)
#define CF_PK_MUL24(a, b) __umul24((a), (b))
#else
#define CF_PK_MUL24(a, b) ((a)*(b))
#endif

// product of two signed operands that fit 24 bits
#if defined(__HIP_DEVICE_COMPILE__)
#define CF_PK_MUL24S(a, b) __mul24((a), (b))
#else
#define CF_PK_MUL24S(a, b) ((a)*(b))
#endif

// ---- a texel's key against one palette entry ----
// B = (cc << 7) | w is the entry's constant (cc = sum_c w_c c^2 of its colour, w its interpolation weight), dt the cross
// term sum_c p_c (w_c c).  The key 128 (cc - 2 dt) + w = B - 256 dt orders entries by error, then by weight.
// The search keeps the key itself, one multiply-add of 24-bit operands (dt < 2^23, m256 = -256 from a register), and
// the smallest wins (minimum form).  It equals the negation of (dt << 8) - B maximised over the entries, the form the
// search once had (a - b == -(b - a) in two's complement and max(-x) == -min(x): tests/test_bc7_key_forms.py); no value
// leaves 32 bits (B < 2^30 and 256 dt < 2^30 under both metrics).  That is the perceptual metric's key.
#define CF_BC7_NO_ENTRY 0x3FFFFFFF      // constant of an entry that does not exist: never the minimum
CF_PK int key_min_form(int dt, int m256, int B) { return CF_PK_MUL24S(dt, m256) + B; }

// Unit weights hold the weight in a full byte, B = (cc << 8) | w and the key B - 512 dt: the four weights of a texel row are
// then the low bytes of four keys and leave them by byte permutes (key_row_weights) instead of a shift and an and-or per
// texel.  With the weight in 8 bits below cc: cc = sum_c c^2 <= 4 * 255^2 < 2^18 and dt <= 4 * 255^2, so B < 2^26, 512 dt < 2^27 and
// |key| = |256 (cc - 2 dt) + w| <= 256 * 260100 + 64 < 2^26; -512 and dt fit the 24-bit multiply; an entry that does not
// exist has the key CF_BC7_NO_ENTRY - 512 dt > 2^29, above every real one.  The key's low byte is the weight (<= 64), its
// error part key >> 8 (arithmetic), and a texel outside the subset has the key 0.

// Unit weights take the cross terms of a texel row against an entry from one v_mfma_i32_4x4x4_16b_i8 instead of four
// v_dot4_u32_u8; the fit then runs with the whole wave on, because the instruction needs the lanes that hold its A rows
// switched on.  For texel bytes a_c, palette bytes b_c and a' = a ^ 0x80, b' = b ^ 0x80 read as
// signed bytes (a' = a - 128): sum a_c b_c = sum a'_c b'_c + 128 sum a_c + 128 sum b'_c, for any bytes.  The instruction
// returns D = sum a'b' + C with C = 128 sum_c a_c, so dt = D + 128 sum b' and the key B - F dt (F = 2^fbits: 256, or 512 with
// the weight byte) is base' - F D with base' = B - 128 F (sb - 512), sb = sum_c b_c.  Ranges: D in [-65024, 325636], |D| < 2^19
// and fits the 24-bit multiply; |base'| < 2^26 + 2^25 < 2^27 with F = 512 (< 2^26 with F = 256); F D < 2^28; an entry that
// does not exist keeps CF_BC7_NO_ENTRY and its key CF_BC7_NO_ENTRY - F D stays inside 32 bits and above every real key.
CF_PK int mfma_entry_base(int B, uint32_t sb, int fbits)
{
	return B + (int)(512u << (7 + fbits)) - (int)CF_PK_MUL24(sb, 1u << (7 + fbits));
}

// The search issues the instruction with C = 0 (tests/test_bc7_search_bias.py).  128 sum_c a_c depends on the texel alone,
// not on the entry: without it D' = sum a'b' and a texel's keys all become key' = base' - 512 D' = key + 65536 A_t, with
// A_t = sum_c a_c <= 1020 the sum of the texel's four RAW channels (the A operand is the raw texel, whatever the fit
// codes).  The shift is the same for every entry and for both halves of mode 6, so the winning entry, the tie order and the
// key's low byte (its weight) stay, and a texel outside the subset still has the key 0.  key' >> 8 = (key >> 8) + 256 A_t
// exactly, so an assignment's error grows by 256 sum_{t in subset} A_t: the fit subtracts that once from the constant
// pp_sum (search_pp_fold), in 32-bit modular arithmetic -- pp_sum' may wrap below zero (a dark block: 256 A_t > sum p^2),
// pp_sum' + sum (key' >> 8) is the true error again.  Ranges: |D'| <= 4 * 128^2 = 2^16; key' in (-2^26, 2^27) (key in
// (-2^26, 2^26), 65536 A_t < 2^26); CF_BC7_NO_ENTRY - 512 D' in (2^29, 2^31): above every real key and inside 32 bits;
// both operands of the 24-bit multiply-add (-512, D') fit 24 bits.
// The bias sum_{t in subset} A_t of a fit of the whole block (mode 6, the planes of modes 4 / 5: their channel sets
// hide raw channels from the fit's own sums) is a per-block table word, the sum of the block's 64 raw bytes (<= 16 320 <
// 2^14).  It lives in the upper half of the words of the per-block table of channel extremes, lo | hi << 8, whose upper
// halves were unused (lohi_pack): no LDS is added.
// A partition fit (no rotation; channel set 7 on an opaque block, 15 on one with alpha) has it in its own subset sums.
CF_PK uint32_t lohi_pack(uint32_t lohi, uint32_t rawsum) { return lohi | (rawsum << 16); }
CF_PK uint32_t lohi_rawsum(uint32_t w) { return w >> 16; }
CF_PK uint32_t lohi_hi(uint32_t w) { return (w >> 8) & 255u; }
// n: texels of the subset; opaque: the fit does not code alpha (s3 = 0), the raw alpha is the constant 255
CF_PK uint32_t search_bias_part(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t n, bool opaque)
{
	return s0 + s1 + s2 + s3 + (opaque ? CF_PK_MUL24(n, 255u) : 0u);
}
CF_PK uint32_t search_pp_fold(uint32_t pp_sum, uint32_t bias) { return pp_sum - (bias << 8); }

// An assignment's error from the SUM of its texels' masked keys instead of a shift and an add per texel
// (tests/test_bc7_shelved_trims.py).  A key inside the subset is 256 e_t + w_t with e_t = key >> 8 its signed error part
// and w_t in 0..64 its weight byte; outside the subset it is 0.  So sum_t key_t = 256 sum_t e_t + wsum, wsum the sum of
// the assignment's weight bytes (the refit sums' S, or four dot products over the weight words), and
// (ksum - wsum) >> 8 = sum_t e_t exactly: the difference is a multiple of 256.  Ranges, in the manner of search_pp_fold:
// key' < 2^27 with the texel-constant term left out (search_pp_fold), and key' >= 0 there: its error part is
// |p - c|^2 + (256 A_t - |p|^2) over the coded channels and 256 a >= a^2 for a byte.  At most 16 texels, so ksum in
// [0, 2^31) and 0 <= wsum <= 1024 <= ksum's weight part: ksum - wsum = 256 sum e_t stays inside a word, the shift is
// exact, and pp_sum + sum_t e_t is the sum the per-texel form reaches, in the same 32-bit modular arithmetic.  (The
// shift is arithmetic all the same: the identity holds for keys of either sign while the sum fits a signed word.)
CF_PK uint32_t search_key_sum_error(uint32_t pp_sum, uint32_t ksum, uint32_t wsum)
{
	return pp_sum + (uint32_t)((int)(ksum - wsum) >> 8);
}

// Extremes of a subset's projections, two texels per step: a texel outside the subset contributes a quiet NaN, which
// minimum and maximum pass over (fminf / fmaxf return the other operand; v_min3_f32 / v_max3_f32 likewise), so one select
// per texel replaces two.  Against the scan that selects after every fminf the value is the same; only where the
// extreme is a zero met with both signs can the SIGN differ, since the order of the comparisons differs and +0 == -0.
// A subset whose projections are all equal has tmin == tmax == that value; an empty one keeps the start values.
// The sign of a zero extreme reaches no payload byte: tmin and tmax feed (tmax - tmin) frac, tmin + d and
// fmaf(axis, t, mean), whose values agree for +0 and -0 except again in the sign of a zero, and clamp255 and the
// quantiser's rounding map both zeros to code 0 (tests/test_bc7_shelved_trims.py, tests/test_gpu_bc7_shelved_trims.py).
CF_PK float proj_or_nan(float t, bool in_subset) { return in_subset ? t : __builtin_nanf(""); }
CF_PK void proj_extremes2(float& tmin, float& tmax, float a, float b)
{
	tmin = __builtin_fminf(__builtin_fminf(tmin, a), b);
	tmax = __builtin_fmaxf(__builtin_fmaxf(tmax, a), b);
}

// The low bytes of four keys as the bytes of one word (a key's low byte is its weight, 0 for a texel outside the subset).
// Two byte permutes and an or on the device.
CF_PK uint32_t key_row_weights(uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3)
{
#if defined(__HIP_DEVICE_COMPILE__)
	// (selector bytes 0..3 address the second operand, 4..7 the first, 0x0C gives a zero byte)
	return __builtin_amdgcn_perm(k1, k0, 0x0C0C0400u) | __builtin_amdgcn_perm(k3, k2, 0x04000C0Cu);
#else
	return (k0 & 255u) | ((k1 & 255u) << 8) | ((k2 & 255u) << 16) | ((k3 & 255u) << 24);
#endif
}

// Dequantise one t-bit code v < 2^t (t = 4..8) to a byte: (v << (8 - t)) | (v >> (2t - 8)).
// v * (2^t + 1) holds v twice, t bits apart and without overlap; the shift drops what falls below the byte.
CF_PK uint32_t dequant1(uint32_t v, uint32_t t)
{
	return CF_PK_MUL24(v, (1u << t) + 1u) >> (2u*t - 8u);
}

// The three colour bytes of a code word at once (t = 4..8 bits each).  The left shift never leaves its byte
// (a code is below 2^t); the mask removes what the right shift carries in from the byte above.  Byte 3 comes out as 0.
CF_PK uint32_t dequant_rgb(uint32_t word, uint32_t t)
{
	const uint32_t c3 = word & 0x00FFFFFFu;
	const uint32_t low = ((1u << (8u - t)) - 1u)*0x010101u;
	return (c3 << (8u - t)) | ((c3 >> (2u*t - 8u)) & low);
}

// All four bytes of a code word: dequant_rgb on the colours, dequant1 on the alpha byte.  tc, ta: total bits of a
// colour / the alpha code (field + p-bit); 0 = the channel is not coded and comes out as 0, whatever its byte holds.
// Everything but the word depends on (tc, ta) alone: calls that share them share the shift counts, the mask and the multiplier.
CF_PK uint32_t dequant_word(uint32_t word, uint32_t tc, uint32_t ta)
{
	const uint32_t coded = (tc ? 0x00FFFFFFu : 0u) | (ta ? 0xFF000000u : 0u);
	return (dequant_rgb(word, tc ? tc : 8u) | (dequant1(word >> 24, ta ? ta : 8u) << 24)) & coded;
}

// Code word of a word of quantised fields: every byte shifted up by S (0 or 1) with the p-bit P below it.
// A field of a p-bit mode has at most 7 bits, so no byte reaches its neighbour.
CF_PK uint32_t code_word(uint32_t qword, uint32_t S, uint32_t P)
{
	return (qword << S) | (P ? 0x01010101u : 0u);
}

// Palette entry of weight w (0..64) between two dequantised endpoint words, every channel
// (iw*e0 + w*e1 + 32) >> 6 with iw = 64 - w: two channels per multiply on 0x00FF00FF pairs.  A channel's
// sum is at most 64*255 + 32 < 2^16, so the halves of a pair never meet, and every operand fits 24 bits.
// The kernel computes it in difference form (pal_line / pal_at below); this is the packed definition the tests hold that
// form and the matrix-pipe identities against.
CF_PK uint32_t pal_word(uint32_t e0, uint32_t e1, uint32_t w)
{
	const uint32_t iw = 64u - w;
	const uint32_t m = 0x00FF00FFu, half = 0x00200020u;
	const uint32_t rb = CF_PK_MUL24(iw, e0 & m) + CF_PK_MUL24(w, e1 & m) + half;
	const uint32_t ga = CF_PK_MUL24(iw, (e0 >> 8) & m) + CF_PK_MUL24(w, (e1 >> 8) & m) + half;
	return ((rb >> 6) & m) | ((ga << 2) & ~m);
}

// The same palette in difference form.  With a = e0 & m and b = e1 & m a pair's sum is
// iw*a + w*b + half = (64*a + half) + w*(b - a): what stands in front of w is the same for every entry of a fit.
// A half of b - a may be negative and then borrows from the half above it, but the true sum is non-negative and
// below 2^32, and both sides agree mod 2^32: unsigned arithmetic gives it exactly.  The line of a fit is formed
// once per assignment; an entry then costs one multiply and one add per channel pair.
struct PalLine { uint32_t rb0, rbd, ga0, gad; };

CF_PK PalLine pal_line(uint32_t e0, uint32_t e1)
{
	const uint32_t m = 0x00FF00FFu, half = 0x00200020u;
	const uint32_t a_rb = e0 & m, a_ga = (e0 >> 8) & m;
	PalLine l;
	l.rb0 = (a_rb << 6) + half; l.rbd = (e1 & m) - a_rb;
	l.ga0 = (a_ga << 6) + half; l.gad = ((e1 >> 8) & m) - a_ga;
	return l;
}

CF_PK uint32_t pal_at(const PalLine& l, uint32_t w)
{
	const uint32_t m = 0x00FF00FFu;
	// (w*d needs the full 32-bit product: d's upper half carries the borrow)
	const uint32_t rb = l.rb0 + w*l.rbd;
	const uint32_t ga = l.ga0 + w*l.gad;
	return ((rb >> 6) & m) | ((ga << 2) & ~m);
}

// The interpolation weights ((k*64 + d/2)/d, d = 2^ib - 1) of a fit's up to eight palette entries as bytes of two
// words.  Rows: index width 2 (entries 4..7 do not exist: weight 0), index width 3, and the two halves of mode 6's
// sixteen entries, which a lane pair shares.
#define CF_BC7_WEIGHT_ROWS 4u
constexpr uint32_t cf_bc7_weight(uint32_t ib, uint32_t k)
{
	return (k*64u + (((1u << ib) - 1u) >> 1))/((1u << ib) - 1u);
}
struct cf_bc7_weight_table { uint32_t w[CF_BC7_WEIGHT_ROWS][2]; };
constexpr cf_bc7_weight_table cf_bc7_make_weights()
{
	cf_bc7_weight_table t = {};
	for (uint32_t k = 0; k < 8u; ++k) {
		t.w[0][k >> 2] |= (k < 4u ? cf_bc7_weight(2u, k) : 0u) << (8u*(k & 3u));
		t.w[1][k >> 2] |= cf_bc7_weight(3u, k) << (8u*(k & 3u));
		t.w[2][k >> 2] |= cf_bc7_weight(4u, k) << (8u*(k & 3u));
		t.w[3][k >> 2] |= cf_bc7_weight(4u, 8u + k) << (8u*(k & 3u));
	}
	return t;
}
// Row of a fit: mode 6's half, or the index width (a width that is neither 2 nor 3 belongs to a lane without a fit
// and reads row 0: the index never leaves the table).
CF_PK uint32_t weight_row(bool m6, uint32_t khalf, uint32_t ib)
{
	return m6 ? 2u + (khalf & 1u) : (ib == 3u ? 1u : 0u);
}
// Entry k = 0..7 of a row's two words
CF_PK uint32_t weight_at(uint32_t w03, uint32_t w47, uint32_t k)
{
	return ((k < 4u ? w03 : w47) >> (8u*(k & 3u))) & 255u;
}

// ---- packed integer moments ----
// The 14 integer moments of a set of texels (channel sums s_c, sums of products q_cd) in 10 words, as the per-block
// table of bc7_encode.hip holds the whole block's: words 0..3 = q_cc | s_c << 20 (q <= 16 * 255^2 < 2^20,
// s <= 16 * 255 < 2^12), words 4..9 = q01 q02 q03 q12 q13 q23.
#define CF_MOM_WORDS 10

// Moments of a set minus those of a subset of it, on the packed words: every field of the subset is at most the set's
// field (sums of non-negative terms over fewer texels), so no field borrows from its neighbour.
CF_PK void mom_sub(const uint32_t (&T)[CF_MOM_WORDS], const uint32_t (&A)[CF_MOM_WORDS], uint32_t (&W)[CF_MOM_WORDS])
{
	for (int m = 0; m < CF_MOM_WORDS; ++m)
		W[m] = T[m] - A[m];
}

// Moments of a fit that covers the whole block, from the block's table words T: the channels as the fit sees them,
// rotation rot (0..3: colour rot - 1 and alpha change places) and channel set chm applied (7: the vector plane,
// slot 3 not coded; 8: the scalar plane, slot 3 alone; 15: all four, which only fits without rotation have).
// opaque: T holds zeros for every alpha term (the table applies the block's own channel set); the alpha plane such a
// fit reads is the constant 255, so s_a = 255 * 16, q_aa = 255^2 * 16, q_ca = 255 * s_c.
CF_PK void mom_whole(const uint32_t (&T)[CF_MOM_WORDS], bool opaque, uint32_t rot, uint32_t chm, uint32_t (&W)[CF_MOM_WORDS])
{
	// (the table's zeros plus the constant's terms: one multiply-add per word, the factor 0 for a block with alpha)
	const uint32_t k = opaque ? 255u : 0u;
	const uint32_t t3 = opaque ? (1040400u | (4080u << 20)) : T[3];
	const uint32_t t6 = CF_PK_MUL24(T[0] >> 20, k) + T[6];
	const uint32_t t8 = CF_PK_MUL24(T[1] >> 20, k) + T[8];
	const uint32_t t9 = CF_PK_MUL24(T[2] >> 20, k) + T[9];
	const bool vec = (chm & 7u) != 0u, sca = (chm & 8u) != 0u, all = vec && sca;
	// slot c < 3 holds colour c, or alpha when the rotation moved it there; slot 3 holds alpha or colour rot - 1
	const uint32_t d0 = rot == 1u ? t3 : T[0], d1 = rot == 2u ? t3 : T[1], d2 = rot == 3u ? t3 : T[2];
	const uint32_t d3 = rot == 0u ? t3 : (rot == 1u ? T[0] : (rot == 2u ? T[1] : T[2]));
	const uint32_t q01 = rot == 1u ? t8 : (rot == 2u ? t6 : T[4]);
	const uint32_t q02 = rot == 1u ? t9 : (rot == 3u ? t6 : T[5]);
	const uint32_t q12 = rot == 2u ? t9 : (rot == 3u ? t8 : T[7]);
	W[0] = vec ? d0 : 0u; W[1] = vec ? d1 : 0u; W[2] = vec ? d2 : 0u; W[3] = sca ? d3 : 0u;
	W[4] = vec ? q01 : 0u; W[5] = vec ? q02 : 0u; W[7] = vec ? q12 : 0u;
	// products of a colour slot with slot 3: coded by four-channel fits alone, and those are not rotated
	W[6] = all ? t6 : 0u; W[8] = all ? t8 : 0u; W[9] = all ? t9 : 0u;
}

// The packed words apart: channel sums s[4] and the ten products in the order q00 q01 q02 q03 q11 q12 q13 q22 q23 q33
CF_PK void mom_unpack(const uint32_t (&W)[CF_MOM_WORDS], uint32_t (&s)[4], uint32_t (&q)[10])
{
	for (int c = 0; c < 4; ++c)
		s[c] = W[c] >> 20;
	q[0] = W[0] & 0xFFFFFu; q[1] = W[4]; q[2] = W[5]; q[3] = W[6];
	q[4] = W[1] & 0xFFFFFu; q[5] = W[7]; q[6] = W[8];
	q[7] = W[2] & 0xFFFFFu; q[8] = W[9];
	q[9] = W[3] & 0xFFFFFu;
}

// Minimum and maximum of the four bytes of a word, as lo | hi << 8
CF_PK uint32_t byte_lohi(uint32_t w)
{
	const uint32_t b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u, b3 = w >> 24;
	uint32_t lo = b0 < b1 ? b0 : b1, hi = b0 > b1 ? b0 : b1;
	lo = b2 < lo ? b2 : lo; hi = b2 > hi ? b2 : hi;
	lo = b3 < lo ? b3 : lo; hi = b3 > hi ? b3 : hi;
	return lo | (hi << 8);
}

// One covariance term n q_cd - s_c s_d as a float, from floats.  n q <= 16 * 16 * 255^2 and s_c s_d <= 4080^2 are both
// 16 646 400 < 2^24: the conversions and the product are exact, and the fused result is an integer below 2^24 in
// magnitude, so it is the float the integer subtraction and its conversion give (+0 where the two are equal).
CF_PK float cov_term(float fn, uint32_t q, float sc, float sd)
{
	return __builtin_fmaf(fn, (float)q, -(sc*sd));
}

// A fit's bytes in a weight word of a candidate's column, which its fits share, as two masks: `keep` clears the bytes
// of the fit's texels (and), `set` puts the new ones in (or).  The fits of a candidate own disjoint texels, so the ands
// and ors of several fits give the same word in any order, each and before its own or, as LDS atomics do for the lanes
// of one wave.
struct cf_put_masks { uint32_t keep, set; };
// rr: the row of the block, w: the fit's weight bytes of that row (zero outside its texels)
CF_PK cf_put_masks cf_put_weights(uint32_t mask, uint32_t rr, uint32_t w)
{
	cf_put_masks m;
	m.keep = ~(((((mask >> (4u*rr)) & 15u)*0x00204081u) & 0x01010101u)*0xFFu);   // (bytemask4 of the row's four mask bits)
	m.set = w;
	return m;
}

#endif
