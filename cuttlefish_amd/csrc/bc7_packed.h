// BC7 endpoint arithmetic on whole code words (bytes r,g,b,a) instead of one channel at a time.
// Plain integer functions: the kernels of bc7_encode.hip use them on the device, a host program can
// include this file and compare them with the per-byte formulas (tests/test_bc7_packed_identities.py).
// Every identity here is exact, so the encoder's payloads do not depend on which form computes them.
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
CF_PK uint32_t pal_word(uint32_t e0, uint32_t e1, uint32_t w)
{
	const uint32_t iw = 64u - w;
	const uint32_t m = 0x00FF00FFu, half = 0x00200020u;
	const uint32_t rb = CF_PK_MUL24(iw, e0 & m) + CF_PK_MUL24(w, e1 & m) + half;
	const uint32_t ga = CF_PK_MUL24(iw, (e0 >> 8) & m) + CF_PK_MUL24(w, (e1 >> 8) & m) + half;
	return ((rb >> 6) & m) | ((ga << 2) & ~m);
}

#endif
