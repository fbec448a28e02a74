// cf_texel.h -- the texel vocabulary of the image passes: how big a pixel is, how a component of
// an RGBA8 / RGBA16F / RGBA32F texel becomes a float, how a unit value is stored back, and how a coordinate wraps.  These
// few lines are the definition of what the library reads and writes; the numpy twins in tests/*_ref.py restate them and
// the tests pin them bit for bit.  A pass includes this header and spells none of them itself.
//
//   decode   RGBA8 (float)((double)v / 255.0), through a 256-entry table a workgroup fills once; RGBA16F half -> float
//            (exact); RGBA32F as stored.  No special-value rule: what a pass makes of a NaN or an infinity is its own
//   store    of a unit value v, a double in [0, 1]: RGBA8 (uint8)floor(v*255.0 + 0.5); RGBA32F (float)v; RGBA16F the
//            nearest-even half of (float)v
//   wrap     a coordinate of a wrapped axis is taken modulo the side (floor modulo: -1 is side - 1)
// Everything above the __HIPCC__ part is a pure function of bits and compiles with a host compiler alone
// (tools/texel_host.cpp, tests/test_texel_host.py).
#ifndef CF_TEXEL_H
#define CF_TEXEL_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/cuttlefish_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CFTX_FN __host__ __device__ inline
#else
#define CFTX_FN inline
#endif

// Bytes of a texel.  Of a type an entry point has checked: here, as in cf_pixel_dispatch, what is neither RGBA8 nor
// RGBA32F is RGBA16F (a fourth arm costs the kernels that store by run-time type registers and instructions).
CFTX_FN constexpr uint32_t cf_pixel_size(int type)
{
	return type == CFHIP_PIXEL_RGBA8 ? 4u : type == CFHIP_PIXEL_RGBA32F ? 16u : 8u;
}

// the only two places that look inside a half
CFTX_FN float cf_half_to_float(uint32_t bits)
{
	union { unsigned short u; _Float16 f; } c;
	c.u = (unsigned short)bits;
	return (float)c.f;
}

CFTX_FN uint16_t cf_float_to_half(float v)
{
	union { unsigned short u; _Float16 f; } c;
	c.f = (_Float16)v;                                 // nearest-even
	return c.u;
}

// Image::convert RGBA8 -> RGBAF of the reference: toDoubleNorm (v/255.0), float store
CFTX_FN float cf_u8_to_float(uint32_t v)
{
	return (float)((double)v/255.0);
}

// with (float)v and cf_float_to_half((float)v), the three stored forms of a unit value
CFTX_FN uint8_t cf_unit_to_u8(double v)
{
	return (uint8_t)floor(v*255.0 + 0.5);
}

CFTX_FN int32_t cf_floor_mod(int32_t v, uint32_t n)
{
	const int32_t m = v % (int32_t)n;
	return m < 0 ? m + (int32_t)n : m;
}

// a coordinate on an axis of `side` texels: modulo the side on a wrapped axis; false where there is no texel
CFTX_FN bool cf_wrap_coord(int32_t& at, uint32_t side, bool wrap)
{
	if (!wrap)
		return at >= 0 && at < (int32_t)side;
	at = cf_floor_mod(at, side);
	return true;
}

// f(std::integral_constant<int, PIX>{}) for the pixel type of a call: the one ladder from a run-time type to a template
// argument.  The type was checked by the entry point; what is neither RGBA8 nor RGBA32F is RGBA16F.
template <class F>
CFTX_FN auto cf_pixel_dispatch(int type, F&& f)
{
	if (type == CFHIP_PIXEL_RGBA8)
		return f(std::integral_constant<int, CFHIP_PIXEL_RGBA8>{});
	if (type == CFHIP_PIXEL_RGBA32F)
		return f(std::integral_constant<int, CFHIP_PIXEL_RGBA32F>{});
	return f(std::integral_constant<int, CFHIP_PIXEL_RGBA16F>{});
}

#if defined(__HIPCC__)
// ---- the device side ----------------------------------------------------------------------------------------------------
// The pixel type is a template argument.  cf_channel_of_raw and cf_store_unit also take it at run time; cf_load_channel does
// not: a kernel that reads one component by run-time type writes its three-way `if` itself, RGBA8 first, around the
// template form -- out of a helper the ladder was lowered as a switch, two more scalar branches on the RGBA8 path, and
// the one-texel-per-thread kernels showed it (profiles/texel_vocabulary_ab.txt).

// the table of the 256 values of an 8-bit component, one entry per thread of a 256-thread workgroup.  The barrier is the
// caller's: most kernels have other LDS to initialise before the same one.
__device__ __forceinline__ void cf_fill_of_u8(float* of_u8, uint32_t thread, bool wanted)
{
	if (wanted)
		of_u8[thread] = cf_u8_to_float(thread);
}

// component ch of texel x of a row: the stored bits, zero-extended
template <int PIX>
__device__ __forceinline__ uint32_t cf_channel_raw(const uint8_t* row, uint32_t x, uint32_t ch)
{
	if (PIX == CFHIP_PIXEL_RGBA8)
		return row[(size_t)x*4u + ch];
	if (PIX == CFHIP_PIXEL_RGBA32F)
		return *reinterpret_cast<const uint32_t*>(row + (size_t)x*16u + ch*4u);
	return *reinterpret_cast<const unsigned short*>(row + (size_t)x*8u + ch*2u);
}

// ... and the float they stand for
template <int PIX>
__device__ __forceinline__ float cf_channel_of_raw(uint32_t raw, const float* of_u8)
{
	if (PIX == CFHIP_PIXEL_RGBA8)
		return of_u8[raw];
	if (PIX == CFHIP_PIXEL_RGBA32F)
		return __uint_as_float(raw);
	return cf_half_to_float(raw);
}

template <int PIX>
__device__ __forceinline__ float cf_load_channel(const uint8_t* row, uint32_t x, uint32_t ch, const float* of_u8)
{
	return cf_channel_of_raw<PIX>(cf_channel_raw<PIX>(row, x, ch), of_u8);
}

__device__ __forceinline__ float cf_channel_of_raw(int type, uint32_t raw, const float* of_u8)
{
	if (type == CFHIP_PIXEL_RGBA8)
		return cf_channel_of_raw<CFHIP_PIXEL_RGBA8>(raw, of_u8);
	if (type == CFHIP_PIXEL_RGBA32F)
		return cf_channel_of_raw<CFHIP_PIXEL_RGBA32F>(raw, of_u8);
	return cf_channel_of_raw<CFHIP_PIXEL_RGBA16F>(raw, of_u8);
}

// the four halves of an RGBA16F texel
__device__ __forceinline__ float4 cf_halves_to_float4(uint2 h)
{
	return make_float4(cf_half_to_float(h.x & 0xFFFFu), cf_half_to_float(h.x >> 16), cf_half_to_float(h.y & 0xFFFFu),
		cf_half_to_float(h.y >> 16));
}

// A whole texel, straight-line code.  WORD: the texel is read as one word of its size, so the row and its pitch are
// aligned to that; without, component by component (four cf_load_channel), at any alignment the components allow.
template <int PIX, bool WORD = true>
__device__ __forceinline__ float4 cf_load_texel(const uint8_t* row, uint32_t x, const float* of_u8)
{
	if (!WORD)
		return make_float4(cf_load_channel<PIX>(row, x, 0u, of_u8), cf_load_channel<PIX>(row, x, 1u, of_u8),
			cf_load_channel<PIX>(row, x, 2u, of_u8), cf_load_channel<PIX>(row, x, 3u, of_u8));
	if (PIX == CFHIP_PIXEL_RGBA8) {
		const uint32_t v = *reinterpret_cast<const uint32_t*>(row + (size_t)x*4u);
		return make_float4(of_u8[v & 255u], of_u8[(v >> 8) & 255u], of_u8[(v >> 16) & 255u], of_u8[v >> 24]);
	}
	if (PIX == CFHIP_PIXEL_RGBA32F)
		return *reinterpret_cast<const float4*>(row + (size_t)x*16u);
	return cf_halves_to_float4(*reinterpret_cast<const uint2*>(row + (size_t)x*8u));
}

// the same texel where no table is at hand: the reference's RGBAF view of a source image
template <int SRC_PIX>
__device__ __forceinline__ float4 load_rgbaf(const uint8_t* row, uint32_t x)
{
	if (SRC_PIX == CFHIP_PIXEL_RGBA8) {
		const uint32_t p = *reinterpret_cast<const uint32_t*>(row + (size_t)x*4u);
		const uint32_t r = p & 255u, g = (p >> 8) & 255u, b = (p >> 16) & 255u, a = p >> 24;
		return make_float4(cf_u8_to_float(r), cf_u8_to_float(g), cf_u8_to_float(b), cf_u8_to_float(a));
	}
	return cf_load_texel<SRC_PIX>(row, x, nullptr);
}

// Color.h's sRGBToLinear / linearToSRGB (:224-242), in double as the reference computes them
__device__ __forceinline__ double srgb_to_linear(double c)
{
	if (c <= 0.04045)
		return c/12.92;
	return pow((c + 0.055)/1.055, 2.4);
}

__device__ __forceinline__ double linear_to_srgb(double c)
{
	if (c <= 0.0031308)
		return c*12.92;
	return 1.055*pow(c, 1.0/2.4) - 0.055;
}

// entry v of the table cf_load_linear reads: the linear value of an 8-bit sRGB component, as the per-texel call gives it
__device__ __forceinline__ double cf_linear_of_u8(uint32_t v)
{
	return srgb_to_linear((double)cf_u8_to_float(v));
}

// A source texel as linear RGBAF: of an sRGB source (`srgb`) the colour components linearised and stored as float --
// the linear copy of the source is an RGBAF image -- alpha apart; else load_rgbaf.  lin_of_u8: (float)cf_linear_of_u8
// of the 256 values, read for an sRGB RGBA8 source only.
template <int SRC_PIX>
__device__ __forceinline__ float4 cf_load_linear(const uint8_t* row, uint32_t x, bool srgb, const float* lin_of_u8)
{
	float4 p;
	if (SRC_PIX == CFHIP_PIXEL_RGBA8 && srgb) {
		const uint32_t u = *reinterpret_cast<const uint32_t*>(row + (size_t)x*4u);
		p = make_float4(lin_of_u8[u & 255u], lin_of_u8[(u >> 8) & 255u], lin_of_u8[(u >> 16) & 255u], cf_u8_to_float(u >> 24));
	} else {
		p = load_rgbaf<SRC_PIX>(row, x);
		if (srgb) {
			p.x = (float)srgb_to_linear((double)p.x);
			p.y = (float)srgb_to_linear((double)p.y);
			p.z = (float)srgb_to_linear((double)p.z);
		}
	}
	return p;
}

// the unit value v into the components of texel x that `mask` names
__device__ __forceinline__ void cf_store_unit(uint8_t* row, uint32_t x, int type, uint32_t mask, double v)
{
	uint8_t* p = row + (size_t)x*cf_pixel_size(type);
	if (type == CFHIP_PIXEL_RGBA8) {
		const uint8_t q = cf_unit_to_u8(v);
#pragma unroll
		for (uint32_t ch = 0; ch < 4; ++ch)
			if (mask >> ch & 1u)
				p[ch] = q;
	} else if (type == CFHIP_PIXEL_RGBA32F) {
		const float q = (float)v;
#pragma unroll
		for (uint32_t ch = 0; ch < 4; ++ch)
			if (mask >> ch & 1u)
				reinterpret_cast<float*>(p)[ch] = q;
	} else {
		const uint16_t q = cf_float_to_half((float)v);
#pragma unroll
		for (uint32_t ch = 0; ch < 4; ++ch)
			if (mask >> ch & 1u)
				reinterpret_cast<uint16_t*>(p)[ch] = q;
	}
}
#endif // __HIPCC__

#endif
