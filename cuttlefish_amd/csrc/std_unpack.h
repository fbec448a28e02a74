// std_unpack.h -- device code shared by the standard-format unpack kernels (std_unpack.hip) and the fused
// compare of the same formats (compare.hip): how a workgroup reads its run of packed pixels, and the value of
// one pixel as RGBA32F.  The field layout is the exact inverse of std_pack.hip's pack_pixel; the value rules are
// the fixed-function conversions of Vulkan / OpenGL (include/cuttlefish_hip.h states the table).
#ifndef CF_STD_UNPACK_H
#define CF_STD_UNPACK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cfstd {

enum { T_UNORM = 0, T_SNORM = 1, T_UINT = 2, T_INT = 3, T_UFLOAT = 4, T_FLOAT = 5 };
enum {
	F_R4G4 = 1, F_R4G4B4A4, F_B4G4R4A4, F_A4R4G4B4, F_R5G6B5, F_B5G6R5, F_R5G5B5A1,
	F_B5G5R5A1, F_A1R5G5B5, F_R8, F_R8G8, F_R8G8B8, F_B8G8R8, F_R8G8B8A8, F_B8G8R8A8,
	F_A8B8G8R8, F_A2R10G10B10, F_A2B10G10R10, F_R16, F_R16G16, F_R16G16B16, F_R16G16B16A16,
	F_R32, F_R32G32, F_R32G32B32, F_R32G32B32A32, F_B10G11R11, F_E5B9G9R9
};

#ifndef CF_STDU_PER_THREAD
#define CF_STDU_PER_THREAD 2
#endif
constexpr uint32_t kThreads = 256, kPerThread = CF_STDU_PER_THREAD, kPixPerWg = kThreads*kPerThread;

// dwords of LDS a workgroup stages its payload run in: the run, a leading partial dword when the run does not
// start on a dword, and one more so that a lane may always read the dword after its pixel's
template <int BPP>
constexpr uint32_t stage_dwords() { return (BPP & 3) ? kPixPerWg*BPP/4 + 2 : 1; }

typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

// The packed pixels p0 + j*kThreads + tid (j < kPerThread) of a tight payload, BPP bytes each, little endian in
// o[j].x .. o[j].w.  Consecutive lanes hold consecutive pixels.
//   * 4 / 8 / 12 / 16 bytes: one dword .. dwordx4 load per pixel (vec: pixels is aligned to 4 / 8 / 4 / 16 bytes;
//     otherwise byte loads).
//   * 1 / 2 / 3 / 6 bytes: the workgroup's contiguous run is read as aligned dwords into LDS -- the dwords at the
//     two ends of the run that are only partly inside it byte by byte, so nothing outside the run is read -- and
//     every lane picks its bytes from there.  Works for any alignment of pixels.  Contains a __syncthreads().
template <int BPP>
__device__ __forceinline__ void load_pixels(const uint8_t* pixels, uint32_t vec, unsigned long long p0,
	unsigned long long npix, uint32_t tid, uint32_t* stage, uint4 (&o)[kPerThread])
{
	if constexpr ((BPP & 3) == 0) {
#pragma unroll
		for (uint32_t j = 0; j < kPerThread; ++j) {
			const unsigned long long p = p0 + j*kThreads + tid;
			o[j] = make_uint4(0, 0, 0, 0);
			if (p >= npix)
				continue;
			const uint8_t* src = pixels + p*BPP;
			if (vec) {
				if (BPP == 4) o[j].x = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src));
				else if (BPP == 8) {
					const u2v v = __builtin_nontemporal_load(reinterpret_cast<const u2v*>(src));
					o[j].x = v.x; o[j].y = v.y;
				} else if (BPP == 12) {
					const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
					o[j].x = __builtin_nontemporal_load(s); o[j].y = __builtin_nontemporal_load(s + 1);
					o[j].z = __builtin_nontemporal_load(s + 2);
				} else {
					const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(src));
					o[j] = make_uint4(v.x, v.y, v.z, v.w);
				}
			} else {
				uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
				for (int k = 0; k < BPP; ++k)
					w[k >> 2] |= (uint32_t)src[k] << (8*(k & 3));
				o[j] = make_uint4(w[0], w[1], w[2], w[3]);
			}
		}
	} else {
		const unsigned long long left = npix - p0;
		const uint32_t bytes = (uint32_t)(left < kPixPerWg ? left : kPixPerWg)*BPP;
		const uint8_t* run = pixels + p0*BPP;
		const uint32_t lead = (uint32_t)((uintptr_t)run & 3u);
		const uint8_t* a0 = run - lead;                  // dword aligned
		const uint32_t end = lead + bytes;               // the run is bytes [lead, end) from a0
		const uint32_t ndw = (end + 3u) >> 2;
		for (uint32_t i = tid; i < ndw; i += kThreads) {
			const uint32_t b0 = i*4u;
			uint32_t v = 0;
			if (b0 >= lead && b0 + 4u <= end)
				v = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(a0 + b0));
			else {
#pragma unroll
				for (uint32_t k = 0; k < 4; ++k)
					if (b0 + k >= lead && b0 + k < end)
						v |= (uint32_t)a0[b0 + k] << (8u*k);
			}
			stage[i] = v;
		}
		__syncthreads();
#pragma unroll
		for (uint32_t j = 0; j < kPerThread; ++j) {
			const uint32_t off = lead + (j*kThreads + tid)*BPP, w = off >> 2, s = off & 3u;
			const uint32_t s0 = stage[w], s1 = stage[w + 1];
			o[j] = make_uint4(0, 0, 0, 0);
			if (BPP == 6) {
				const uint32_t s2 = stage[w + 2];
				o[j].x = __builtin_amdgcn_alignbyte(s1, s0, s);
				o[j].y = __builtin_amdgcn_alignbyte(s2, s1, s) & 0xFFFFu;
			} else
				o[j].x = __builtin_amdgcn_alignbyte(s1, s0, s) & (0xFFFFFFFFu >> (32 - 8*BPP));
		}
	}
}

// (float)v / (float)MAX, correctly rounded, without the division sequence: q = v*(1/MAX) is within an ulp and one
// Newton step with an exact remainder lands on the rounded quotient.  tests/test_std_unpack_ref.py checks the
// expression against the true quotient for every v of every MAX used here.
template <uint32_t MAX>
__device__ __forceinline__ float quot(float x)
{
	constexpr float d = (float)MAX, r = 1.0f/(float)MAX;
	const float q = x*r;
	return fmaf(fmaf(-q, d, x), r, q);
}

template <uint32_t MAX>
__device__ __forceinline__ float unorm_f(uint32_t v) { return quot<MAX>((float)v); }

template <int BITS>
__device__ __forceinline__ int32_t sext(uint32_t v) { return (int32_t)(v << (32 - BITS)) >> (32 - BITS); }

template <int BITS>
__device__ __forceinline__ float snorm_f(uint32_t v)
{
	return fmaxf(quot<(1u << (BITS - 1)) - 1u>((float)sext<BITS>(v)), -1.0f);
}

__device__ __forceinline__ float half_f(uint32_t h)
{
	union { unsigned short u; _Float16 f; } c;
	c.u = (unsigned short)(h & 0xFFFFu);
	return (float)c.f;
}

// a field of a channel array (R8.., R16.., R32..) under Texture::Type `type`
template <int BITS>
__device__ __forceinline__ float chan(uint32_t v, uint32_t type)
{
	if constexpr (BITS == 32) {
		return type == T_UINT ? (float)v : (type == T_INT ? (float)(int32_t)v : __uint_as_float(v));
	} else {
		v &= (1u << BITS) - 1u;
		switch (type) {
			case T_UNORM: return unorm_f<(1u << BITS) - 1u>(v);
			case T_SNORM: return snorm_f<BITS>(v);
			case T_UINT: return (float)v;
			case T_INT: return (float)sext<BITS>(v);
			default: return BITS == 16 ? half_f(v) : 0.0f;
		}
	}
}

// unsigned small float of B10G11R11: 5 exponent bits (bias 15), MB mantissa bits
template <int MB>
__device__ __forceinline__ float ufloat_f(uint32_t v)
{
	const uint32_t e = (v >> MB) & 31u, m = v & ((1u << MB) - 1u);
	if (e == 0)
		return (float)m*__uint_as_float((uint32_t)(127 - 14 - MB) << 23);      // m * 2^(-14 - MB), exact
	if (e == 31)
		return __uint_as_float(m ? 0x7FC00000u : 0x7F800000u);
	return __uint_as_float(((e + 112u) << 23) | (m << (23 - MB)));
}

// BPP bytes of one pixel (little endian in o.x .. o.w) -> RGBA32F; channels the format does not store: 0, 0, 0, 1
template <int BPP>
__device__ __forceinline__ float4 unpack_pixel(uint32_t format, uint32_t type, uint4 o)
{
	float r = 0.0f, g = 0.0f, b = 0.0f, a = 1.0f;
	const uint32_t v = o.x;
	if constexpr (BPP == 1) {
		if (format == F_R4G4) {
			g = unorm_f<15>(v & 15u); r = unorm_f<15>((v >> 4) & 15u);
		} else
			r = chan<8>(v, type);
	} else if constexpr (BPP == 2) {
		if (format >= F_R4G4B4A4 && format <= F_A4R4G4B4) {
			const float n0 = unorm_f<15>(v & 15u), n1 = unorm_f<15>((v >> 4) & 15u),
				n2 = unorm_f<15>((v >> 8) & 15u), n3 = unorm_f<15>((v >> 12) & 15u);
			g = n2;
			if (format == F_R4G4B4A4) { a = n0; b = n1; r = n3; }
			else if (format == F_B4G4R4A4) { a = n0; r = n1; b = n3; }
			else { b = n0; g = n1; r = n2; a = n3; }
		} else if (format == F_R5G6B5 || format == F_B5G6R5) {
			const float lo = unorm_f<31>(v & 31u), hi = unorm_f<31>((v >> 11) & 31u);
			g = unorm_f<63>((v >> 5) & 63u);
			r = format == F_R5G6B5 ? hi : lo;
			b = format == F_R5G6B5 ? lo : hi;
		} else if (format == F_R5G5B5A1 || format == F_B5G5R5A1) {
			const float lo = unorm_f<31>((v >> 1) & 31u), hi = unorm_f<31>((v >> 11) & 31u);
			a = (float)(v & 1u);
			g = unorm_f<31>((v >> 6) & 31u);
			r = format == F_R5G5B5A1 ? hi : lo;
			b = format == F_R5G5B5A1 ? lo : hi;
		} else if (format == F_A1R5G5B5) {
			b = unorm_f<31>(v & 31u); g = unorm_f<31>((v >> 5) & 31u); r = unorm_f<31>((v >> 10) & 31u);
			a = (float)((v >> 15) & 1u);
		} else if (format == F_R8G8) {
			r = chan<8>(v, type); g = chan<8>(v >> 8, type);
		} else
			r = chan<16>(v, type);                       // R16
	} else if constexpr (BPP == 3) {
		const float c0 = chan<8>(v, type), c1 = chan<8>(v >> 8, type), c2 = chan<8>(v >> 16, type);
		g = c1;
		r = format == F_B8G8R8 ? c2 : c0;
		b = format == F_B8G8R8 ? c0 : c2;
	} else if constexpr (BPP == 4) {
		switch (format) {
			case F_R8G8B8A8: case F_B8G8R8A8: {
				const float c0 = chan<8>(v, type), c2 = chan<8>(v >> 16, type);
				g = chan<8>(v >> 8, type); a = chan<8>(v >> 24, type);
				r = format == F_R8G8B8A8 ? c0 : c2;
				b = format == F_R8G8B8A8 ? c2 : c0;
				break;
			}
			case F_A8B8G8R8:
				a = unorm_f<255>(v & 255u); b = unorm_f<255>((v >> 8) & 255u); g = unorm_f<255>((v >> 16) & 255u);
				r = unorm_f<255>(v >> 24);
				break;
			case F_A2R10G10B10: case F_A2B10G10R10: {
				const uint32_t q0 = v & 1023u, q1 = (v >> 10) & 1023u, q2 = (v >> 20) & 1023u, q3 = v >> 30;
				float c0, c2;
				if (type == T_UNORM) {
					c0 = unorm_f<1023>(q0); g = unorm_f<1023>(q1); c2 = unorm_f<1023>(q2); a = unorm_f<3>(q3);
				} else {
					c0 = (float)q0; g = (float)q1; c2 = (float)q2; a = (float)q3;
				}
				r = format == F_A2R10G10B10 ? c2 : c0;
				b = format == F_A2R10G10B10 ? c0 : c2;
				break;
			}
			case F_R16G16: r = chan<16>(v, type); g = chan<16>(v >> 16, type); break;
			case F_B10G11R11:
				r = ufloat_f<6>(v & 0x7FFu); g = ufloat_f<6>((v >> 11) & 0x7FFu); b = ufloat_f<5>(v >> 22);
				break;
			case F_E5B9G9R9: {
				const float sc = __uint_as_float(((v >> 27) + 103u) << 23);       // 2^(e - 24), e - 24 in [-24, 7]
				r = (float)(v & 0x1FFu)*sc; g = (float)((v >> 9) & 0x1FFu)*sc; b = (float)((v >> 18) & 0x1FFu)*sc;
				break;
			}
			default: r = chan<32>(v, type); break;        // R32
		}
	} else if constexpr (BPP == 6) {
		r = chan<16>(v, type); g = chan<16>(v >> 16, type); b = chan<16>(o.y, type);
	} else if constexpr (BPP == 8) {
		if (format == F_R16G16B16A16) {
			r = chan<16>(v, type); g = chan<16>(v >> 16, type); b = chan<16>(o.y, type); a = chan<16>(o.y >> 16, type);
		} else {
			r = chan<32>(v, type); g = chan<32>(o.y, type);
		}
	} else {
		r = chan<32>(v, type); g = chan<32>(o.y, type); b = chan<32>(o.z, type);
		if (BPP == 16)
			a = chan<32>(o.w, type);
	}
	return make_float4(r, g, b, a);
}

} // namespace cfstd
#endif
