// decode.hip -- GPU decoders of every block format the library encodes, and a fused decode + SSE pass.
//
// Output is bit-identical to the project's CPU oracle decoders (oracle/bcn_decode.c, bc6h_decode.c,
// etc_codec.c, astc_decode.c), which are pinned to Pillow and Mesa through committed fixtures.
//
// Shapes:
//   * BCn / BC7 / BC6H / ETC / EAC: one lane per 4x4 block, adjacent lanes on adjacent blocks of a block
//     row; the block is read with one 8- or 16-byte load and every texel row of it written as one store of
//     4 .. 32 bytes when the output is 16-byte aligned (a byte path otherwise).
//   * ASTC: one workgroup per run of 64 blocks of a block row.  Phase 1: lane b parses block b into an LDS
//     record (unquantised grid weights of both planes, endpoint pairs of up to 4 partitions).  Phase 2: the
//     lanes walk the run's texels row by row -- adjacent lanes on adjacent texels of the image -- and run the
//     weight infill, the partition hash and the interpolation per texel.  Infill and partition are computed
//     from the specification's formulas, so every legal block mode, grid and seed decodes (the encoder's
//     per-footprint tables list only what it emits).
// Batched launches (decode_batch.h): cfhip_decode_batch_kernel / cfhip_decode_batch_astc_kernel
// run the same per-block device functions as the per-surface kernels behind a surface-table lookup, and can store
// RGBA8 / RGBA32F pixels instead of the native layout.
// Error blocks (BC6H reserved modes; ASTC illegal blocks, and HDR endpoints under the LDR profile) are
// counted with one ballot per wave and one 64-bit atomic per workgroup.  The SSE kernels decode the same
// way but compare against an RGBA8 reference instead of storing, and reduce per wave, then per workgroup.
// The per-format block decoders live in decode_blocks.h, shared with the quality metrics (compare.hip).
// No kernel here may use scratch, spill a vector register or use AGPRs (cuttlefish_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_blocks.h"
#include "decode_batch.h"
#include "std_unpack.h"

namespace {

struct cfdec_args {
	const uint8_t* blocks;
	uint8_t* out;                 // decode: texels, out_pitch bytes between rows
	const uint8_t* ref;           // SSE: RGBA8 reference, ref_pitch bytes between rows
	unsigned long long out_pitch, ref_pitch;
	uint32_t width, height, bx, by;
	unsigned long long* acc;      // decode: error-block counter (may be null); SSE: sum[4]
	uint32_t out_vec;             // out / ref and its pitch are 16-byte aligned
	uint32_t blk_vec;             // blocks is aligned to the block size
};

constexpr int kWg = CFDEC_WG;          // threads of the lane-per-block kernels
constexpr int kAstcRun = CFDEC_ASTC_RUN;      // blocks (and threads) of an ASTC workgroup

// ---------------------------------------------------------------- the lane-per-block kernels

// one texel row (4 texels, TB bytes each) of the block's words to the output
template <int TB>
__device__ __forceinline__ void store_row(uint8_t* dst, const uint32_t* w, int j, int n, bool vec)
{
	if (vec && n == 4) {
		if constexpr (TB == 1)
			*reinterpret_cast<uint32_t*>(dst) = w[j];
		else if constexpr (TB == 2)
			*reinterpret_cast<uint2*>(dst) = make_uint2(w[2*j], w[2*j + 1]);
		else if constexpr (TB == 4)
			*reinterpret_cast<uint4*>(dst) = make_uint4(w[4*j], w[4*j + 1], w[4*j + 2], w[4*j + 3]);
		else {
			reinterpret_cast<uint4*>(dst)[0] = make_uint4(w[8*j], w[8*j + 1], w[8*j + 2], w[8*j + 3]);
			reinterpret_cast<uint4*>(dst)[1] = make_uint4(w[8*j + 4], w[8*j + 5], w[8*j + 6], w[8*j + 7]);
		}
		return;
	}
#pragma unroll
	for (int b = 0; b < 4*TB; ++b)
		if (b < n*TB)
			dst[b] = (uint8_t)(w[j*TB + b/4] >> (8*(b & 3)));
}

// A half widened exactly, NaN payloads included: the hardware conversion quiets a signalling NaN, which a raw
// void-extent colour of an ASTC HDR block may be, so infinities and NaNs are widened by hand.
__device__ __forceinline__ float half_wide(uint32_t h)
{
	h &= 0xFFFFu;
	if ((h & 0x7C00u) == 0x7C00u)
		return __uint_as_float(((h & 0x8000u) << 16) | 0x7F800000u | ((h & 0x3FFu) << 13));
	return cfstd::half_f(h);
}

// The words of one OUT pixel from texel (i, j) of a decoded block (w: the block in its native layout).
// CFDEC_OUT_RGBA8: R8 / RG8 UNorm expanded, one word.  CFDEC_OUT_RGBA32F: four floats with the values cfhip_compare
// documents -- v / 255, max(v / 127, -1), EAC v / 2047 and max(v / 1023, -1), halves widened -- each the correctly
// rounded quotient (std_unpack.h quot<>, proved on the CPU for every value of these divisors).
template <int FMT, int TYPE, int OUT>
__device__ __forceinline__ void convert_texel(const uint32_t* w, int i, int j, uint32_t* o)
{
	constexpr int TB = texel_bytes<FMT, TYPE>();
	constexpr bool SN = TYPE == 1;
	if constexpr (OUT == CFDEC_OUT_RGBA8) {
		if constexpr (TB == 1) o[0] = ((w[j] >> (8*i)) & 255u) | 0xFF000000u;
		else o[0] = ((w[2*j + (i >> 1)] >> (16*(i & 1))) & 0xFFFFu) | 0xFF000000u;
	} else {
		float r = 0.0f, g = 0.0f, b = 0.0f, a = 1.0f;
		if constexpr (FMT == 35) {
			r = half_wide(w[8*j + 2*i]); g = half_wide(w[8*j + 2*i] >> 16);
			b = half_wide(w[8*j + 2*i + 1]); a = half_wide(w[8*j + 2*i + 1] >> 16);
		} else if constexpr (FMT == 33) {
			const uint32_t v = (w[j] >> (8*i)) & 255u;
			r = SN ? cfstd::snorm_f<8>(v) : cfstd::unorm_f<255>(v);
		} else if constexpr (FMT == 34) {
			const uint32_t v = (w[2*j + (i >> 1)] >> (16*(i & 1))) & 0xFFFFu;
			r = SN ? cfstd::snorm_f<8>(v & 255u) : cfstd::unorm_f<255>(v & 255u);
			g = SN ? cfstd::snorm_f<8>(v >> 8) : cfstd::unorm_f<255>(v >> 8);
		} else if constexpr (FMT == 41 || FMT == 42) {
			const uint32_t v = FMT == 41 ? (w[2*j + (i >> 1)] >> (16*(i & 1))) & 0xFFFFu : w[4*j + i];
			// signed EAC holds -1023 .. 1023 in 16 bits: the divisor is 1023, not the 16-bit maximum
			r = SN ? fmaxf(cfstd::quot<1023u>((float)cfstd::sext<16>(v & 0xFFFFu)), -1.0f) : cfstd::unorm_f<2047>(v & 0xFFFFu);
			if constexpr (FMT == 42)
				g = SN ? fmaxf(cfstd::quot<1023u>((float)cfstd::sext<16>(v >> 16)), -1.0f) : cfstd::unorm_f<2047>(v >> 16);
		} else {
			const uint32_t v = w[4*j + i];
			r = cfstd::unorm_f<255>(v & 255u); g = cfstd::unorm_f<255>((v >> 8) & 255u);
			b = cfstd::unorm_f<255>((v >> 16) & 255u); a = cfstd::unorm_f<255>(v >> 24);
		}
		o[0] = __float_as_uint(r); o[1] = __float_as_uint(g); o[2] = __float_as_uint(b); o[3] = __float_as_uint(a);
	}
}

// the decoded block at texel (x0, y0) to the surface: native rows, or converted texels
template <int FMT, int TYPE, int OUT>
__device__ __forceinline__ void store_block(const cfdec_args& a, const uint32_t* w, uint32_t x0, uint32_t y0)
{
	constexpr int TB = texel_bytes<FMT, TYPE>();
	if constexpr (OUT == CFDEC_OUT_NATIVE) {
		const int n = a.width - x0 >= 4 ? 4 : (int)(a.width - x0);
#pragma unroll
		for (int j = 0; j < 4; ++j)
			if (y0 + j < a.height)
				store_row<TB>(a.out + (uint64_t)(y0 + j)*a.out_pitch + (uint64_t)x0*TB, w, j, n, a.out_vec != 0);
	} else {
		constexpr int OW = OUT == CFDEC_OUT_RGBA8 ? 1 : 4;      // words per output texel
#pragma unroll
		for (int j = 0; j < 4; ++j)
#pragma unroll
			for (int i = 0; i < 4; ++i)
				if (y0 + j < a.height && x0 + i < a.width) {
					uint32_t o[OW];
					convert_texel<FMT, TYPE, OUT>(w, i, j, o);
					uint8_t* dst = a.out + (uint64_t)(y0 + j)*a.out_pitch + (uint64_t)(x0 + i)*(4*OW);
					if (a.out_vec) {
						if constexpr (OW == 1) *reinterpret_cast<uint32_t*>(dst) = o[0];
						else *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
					} else {
#pragma unroll
						for (int k = 0; k < 4*OW; ++k)
							dst[k] = (uint8_t)(o[k >> 2] >> (8*(k & 3)));
					}
				}
	}
}

// One workgroup of the lane-per-block decoders: this lane decodes block b of the surface `a` describes and stores
// it as OUT; the workgroup's error blocks are added to a.acc.  Every thread of the workgroup must call it.
template <int FMT, int TYPE, int OUT>
__device__ __forceinline__ void block_wg(const cfdec_args& a, uint64_t b)
{
	constexpr int TB = texel_bytes<FMT, TYPE>();
	constexpr int BB = (FMT == 29 || FMT == 30 || FMT == 33 || (FMT >= 37 && FMT <= 39) || FMT == 41) ? 8 : 16;
	__shared__ uint32_t wg_err;
	if (threadIdx.x == 0)
		wg_err = 0;
	__syncthreads();
	const uint64_t nblk = (uint64_t)a.bx*a.by;
	bool err = false;
	if (b < nblk) {
		const uint32_t by = (uint32_t)(b/a.bx), bx = (uint32_t)(b - (uint64_t)by*a.bx);
		uint64_t lo, hi;
		load_block(a.blocks + b*BB, BB, a.blk_vec != 0, lo, hi);
		uint32_t w[4*TB];
		err = decode4x4<FMT, TYPE>(lo, hi, w);
		store_block<FMT, TYPE, OUT>(a, w, bx*4, by*4);
	}
	if (FMT == 35 && a.acc) {
		const uint64_t m = __ballot(err);
		if ((threadIdx.x & 63) == 0 && m)
			atomicAdd(&wg_err, (uint32_t)__popcll(m));
		__syncthreads();
		if (threadIdx.x == 0 && wg_err)
			atomicAdd(a.acc, (unsigned long long)wg_err);
	}
}

template <int FMT, int TYPE>
__global__ __launch_bounds__(kWg) void cfhip_decode_block_kernel(cfdec_args a)
{
	block_wg<FMT, TYPE, CFDEC_OUT_NATIVE>(a, (uint64_t)blockIdx.x*kWg + threadIdx.x);
}

// ---------------------------------------------------------------- batched launches (decode_batch.h)
struct cfdec_batch {
	const cfdec_batch_entry* table;
	unsigned long long* errors;   // one counter per surface, or null
	uint32_t n;
};

// the surface of workgroup wg: a wave-uniform binary search over wg_begin (cf_resolve's, cf_device.h)
__device__ __forceinline__ uint32_t batch_surface(const cfdec_batch& t, uint32_t wg, cfdec_args& a, uint32_t& wgx)
{
	uint32_t lo = 0, hi = t.n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1u) >> 1;
		if (t.table[mid].wg_begin <= wg) lo = mid; else hi = mid - 1u;
	}
	const cfdec_batch_entry e = t.table[lo];
	a.blocks = e.blocks; a.out = e.out; a.ref = nullptr;
	a.out_pitch = e.out_pitch; a.ref_pitch = 0;
	a.width = e.width; a.height = e.height; a.bx = e.bx; a.by = e.by;
	a.acc = t.errors ? t.errors + lo : nullptr;
	a.out_vec = e.out_vec; a.blk_vec = e.blk_vec;
	wgx = e.wgx;
	return wg - e.wg_begin;
}

template <int FMT, int TYPE, int OUT>
__global__ __launch_bounds__(kWg) void cfhip_decode_batch_kernel(cfdec_batch t)
{
	cfdec_args a;
	uint32_t wgx;
	const uint32_t local = batch_surface(t, blockIdx.x, a, wgx);
	block_wg<FMT, TYPE, OUT>(a, (uint64_t)local*kWg + threadIdx.x);
}

// reference texel (RGBA8) at (x, y)
__device__ __forceinline__ uint32_t ref_texel(const cfdec_args& a, uint32_t x, uint32_t y)
{
	const uint8_t* p = a.ref + (uint64_t)y*a.ref_pitch + (uint64_t)x*4;
	if (a.out_vec)
		return *reinterpret_cast<const uint32_t*>(p);
	return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ void sse_add(uint32_t* s, uint32_t dec, uint32_t ref, int channels)
{
#pragma unroll
	for (int c = 0; c < 4; ++c)
		if (c < channels) {
			const int d = (int)((dec >> (8*c)) & 255u) - (int)((ref >> (8*c)) & 255u);
			s[c] += (uint32_t)(d*d);
		}
}

// per-wave sums, then one 64-bit atomic per workgroup and channel
template <int NT>
__device__ __forceinline__ void sse_reduce(const uint32_t* s, unsigned long long* acc)
{
	__shared__ unsigned long long wg[4];
	if (threadIdx.x < 4)
		wg[threadIdx.x] = 0;
	__syncthreads();
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		const unsigned long long v = wave_sum((unsigned long long)s[c]);
		if ((threadIdx.x & 63) == 0 && v)
			atomicAdd(&wg[c], v);
	}
	__syncthreads();
	if (threadIdx.x < 4 && wg[threadIdx.x])
		atomicAdd(acc + threadIdx.x, wg[threadIdx.x]);
}

template <int FMT, int TYPE>
__global__ __launch_bounds__(kWg) void cfhip_decode_sse_block_kernel(cfdec_args a)
{
	constexpr int TB = texel_bytes<FMT, TYPE>();
	constexpr int BB = (FMT == 29 || FMT == 30 || FMT == 33 || (FMT >= 37 && FMT <= 39) || FMT == 41) ? 8 : 16;
	constexpr int CH = FMT == 33 ? 1 : (FMT == 34 ? 2 : 4);
	const uint64_t b = (uint64_t)blockIdx.x*kWg + threadIdx.x;
	const uint64_t nblk = (uint64_t)a.bx*a.by;
	uint32_t s[4] = {0u, 0u, 0u, 0u};
	if (b < nblk) {
		const uint32_t by = (uint32_t)(b/a.bx), bx = (uint32_t)(b - (uint64_t)by*a.bx);
		uint64_t lo, hi;
		load_block(a.blocks + b*BB, BB, a.blk_vec != 0, lo, hi);
		uint32_t w[4*TB];
		decode4x4<FMT, TYPE>(lo, hi, w);
		const uint32_t x0 = bx*4, y0 = by*4;
#pragma unroll
		for (int j = 0; j < 4; ++j)
#pragma unroll
			for (int i = 0; i < 4; ++i)
				if (y0 + j < a.height && x0 + i < a.width) {
					uint32_t d;
					if constexpr (TB == 4) d = w[4*j + i];
					else if constexpr (TB == 1) d = (w[j] >> (8*i)) & 255u;
					else d = (w[2*j + (i >> 1)] >> (16*(i & 1))) & 0xFFFFu;
					sse_add(s, d, ref_texel(a, x0 + i, y0 + j), CH);
				}
	}
	sse_reduce<kWg>(s, a.acc);
}

// one workgroup = a run of kAstcRun blocks of one block row; grid (ceil(bx / kAstcRun), by)
template <bool HDR, bool SSE, int OUT = CFDEC_OUT_NATIVE>
__device__ __forceinline__ void astc_body(const cfdec_args& a, int bw, int bh, uint32_t run, uint32_t by)
{
	__shared__ AstcRec rec[kAstcRun];
	const uint32_t run0 = run*kAstcRun;
	const uint32_t nb = a.bx - run0 < (uint32_t)kAstcRun ? a.bx - run0 : (uint32_t)kAstcRun;
	if (threadIdx.x < nb) {
		const uint8_t* p = a.blocks + ((uint64_t)by*a.bx + run0 + threadIdx.x)*16u;
		uint64_t lo, hi;
		load_block(p, 16, a.blk_vec != 0, lo, hi);
		astc_parse(lo, hi, bw, bh, HDR, rec[threadIdx.x]);
	}
	__syncthreads();
	// phase 2: the run's texels row by row, adjacent lanes on adjacent texels
	const uint32_t x0 = run0*bw, y0 = by*bh;
	const uint32_t rw = (a.width - x0 < nb*bw) ? a.width - x0 : nb*bw;
	const uint32_t rh = (a.height - y0 < (uint32_t)bh) ? a.height - y0 : (uint32_t)bh;
	const uint32_t total = rw*rh;
	uint32_t s[4] = {0u, 0u, 0u, 0u};
	for (uint32_t k = threadIdx.x; k < total; k += kAstcRun) {
		const uint32_t ty = k/rw, tx = k - ty*rw;
		const uint32_t blk = tx/bw, ts = tx - blk*bw;
		uint32_t o[2];
		astc_texel<HDR>(rec[blk], bw, bh, (int)ts, (int)ty, o);
		const uint32_t X = x0 + tx, Y = y0 + ty;
		if (SSE) {
			sse_add(s, o[0], ref_texel(a, X, Y), 4);
		} else if constexpr (OUT == CFDEC_OUT_RGBA32F) {
			float f[4];
			if (HDR) {
				f[0] = half_wide(o[0]); f[1] = half_wide(o[0] >> 16);
				f[2] = half_wide(o[1]); f[3] = half_wide(o[1] >> 16);
			} else {
#pragma unroll
				for (int c = 0; c < 4; ++c)
					f[c] = cfstd::unorm_f<255>((o[0] >> (8*c)) & 255u);
			}
			uint8_t* dst = a.out + (uint64_t)Y*a.out_pitch + (uint64_t)X*16u;
			if (a.out_vec) {
				*reinterpret_cast<float4*>(dst) = make_float4(f[0], f[1], f[2], f[3]);
			} else {
#pragma unroll
				for (int b = 0; b < 16; ++b)
					dst[b] = (uint8_t)(__float_as_uint(f[b >> 2]) >> (8*(b & 3)));
			}
		} else {
			uint8_t* dst = a.out + (uint64_t)Y*a.out_pitch + (uint64_t)X*(HDR ? 8 : 4);
			if (a.out_vec) {
				if (HDR) *reinterpret_cast<uint2*>(dst) = make_uint2(o[0], o[1]);
				else *reinterpret_cast<uint32_t*>(dst) = o[0];
			} else {
#pragma unroll
				for (int b = 0; b < (HDR ? 8 : 4); ++b)
					dst[b] = (uint8_t)(o[b >> 2] >> (8*(b & 3)));
			}
		}
	}
	if (SSE) {
		sse_reduce<kAstcRun>(s, a.acc);
		return;
	}
	if (!a.acc)
		return;
	__syncthreads();
	const bool err = threadIdx.x < nb && (rec[threadIdx.x].status < 0 || rec[threadIdx.x].bad);
	const uint64_t m = __ballot(err);
	if (threadIdx.x == 0 && m)
		atomicAdd(a.acc, (unsigned long long)__popcll(m));
}

template <bool HDR>
__global__ __launch_bounds__(kAstcRun) void cfhip_decode_astc_kernel(cfdec_args a, int bw, int bh)
{
	astc_body<HDR, false>(a, bw, bh, blockIdx.x, blockIdx.y);
}

template <bool HDR, int OUT>
__global__ __launch_bounds__(kAstcRun) void cfhip_decode_batch_astc_kernel(cfdec_batch t, int bw, int bh)
{
	cfdec_args a;
	uint32_t wgx;
	const uint32_t local = batch_surface(t, blockIdx.x, a, wgx);
	const uint32_t by = local/wgx;
	astc_body<HDR, false, OUT>(a, bw, bh, local - by*wgx, by);
}

__global__ __launch_bounds__(kAstcRun) void cfhip_decode_sse_astc_kernel(cfdec_args a, int bw, int bh)
{
	astc_body<false, true>(a, bw, bh, blockIdx.x, blockIdx.y);
}

template <int FMT, int TYPE>
hipError_t launch4x4(const cfdec_args& a, bool sse, hipStream_t stream)
{
	const uint64_t nblk = (uint64_t)a.bx*a.by;
	const dim3 grid((uint32_t)((nblk + kWg - 1)/kWg)), block(kWg);
	if (sse)
		hipLaunchKernelGGL((cfhip_decode_sse_block_kernel<FMT, TYPE>), grid, block, 0, stream, a);
	else
		hipLaunchKernelGGL((cfhip_decode_block_kernel<FMT, TYPE>), grid, block, 0, stream, a);
	return hipGetLastError();
}

} // namespace

// Host launcher (cfhip_api.hip checks every argument first).  format / type: a (format, type) pair whose decoded
// layout exists; sse: the fused SSE kernel (RGBA8, R8 and RG8 UNorm layouts only).  acc: error-block counter
// (decode, may be null) or the four sums (SSE).
extern "C" hipError_t cfhip_launch_decode(int format, int type, const void* blocks, int blk_vec, void* out,
	size_t out_pitch, const void* ref, size_t ref_pitch, int out_vec, uint32_t width, uint32_t height,
	uint32_t bx, uint32_t by, int bw, int bh, unsigned long long* acc, int sse, hipStream_t stream)
{
	cfdec_args a;
	a.blocks = static_cast<const uint8_t*>(blocks);
	a.out = static_cast<uint8_t*>(out);
	a.ref = static_cast<const uint8_t*>(ref);
	a.out_pitch = out_pitch;
	a.ref_pitch = ref_pitch;
	a.width = width; a.height = height; a.bx = bx; a.by = by;
	a.acc = acc;
	a.out_vec = (uint32_t)out_vec;
	a.blk_vec = (uint32_t)blk_vec;
	if (format >= 43 && format <= 56) {
		const dim3 grid((bx + kAstcRun - 1)/kAstcRun, by), block(kAstcRun);
		if (sse)
			hipLaunchKernelGGL(cfhip_decode_sse_astc_kernel, grid, block, 0, stream, a, bw, bh);
		else if (type == 4)
			hipLaunchKernelGGL(cfhip_decode_astc_kernel<true>, grid, block, 0, stream, a, bw, bh);
		else
			hipLaunchKernelGGL(cfhip_decode_astc_kernel<false>, grid, block, 0, stream, a, bw, bh);
		return hipGetLastError();
	}
	const bool s = sse != 0, sn = type == 1;
	switch (format) {
		case 29: return launch4x4<29, 0>(a, s, stream);
		case 30: return launch4x4<30, 0>(a, s, stream);
		case 31: return launch4x4<31, 0>(a, s, stream);
		case 32: return launch4x4<32, 0>(a, s, stream);
		case 33: return sn ? launch4x4<33, 1>(a, false, stream) : launch4x4<33, 0>(a, s, stream);
		case 34: return sn ? launch4x4<34, 1>(a, false, stream) : launch4x4<34, 0>(a, s, stream);
		case 35: return type == 5 ? launch4x4<35, 5>(a, false, stream) : launch4x4<35, 4>(a, false, stream);
		case 36: return launch4x4<36, 0>(a, s, stream);
		case 37: return launch4x4<37, 0>(a, s, stream);
		case 38: return launch4x4<38, 0>(a, s, stream);
		case 39: return launch4x4<39, 0>(a, s, stream);
		case 40: return launch4x4<40, 0>(a, s, stream);
		case 41: return sn ? launch4x4<41, 1>(a, false, stream) : launch4x4<41, 0>(a, false, stream);
		case 42: return sn ? launch4x4<42, 1>(a, false, stream) : launch4x4<42, 0>(a, false, stream);
		default: return hipErrorInvalidValue;
	}
}

namespace {

template <int FMT, int TYPE>
hipError_t launch_batch4x4(const cfdec_batch& t, int out, uint32_t total_wg, hipStream_t stream)
{
	constexpr int TB = texel_bytes<FMT, TYPE>();
	const dim3 grid(total_wg), block(kWg);
	if (out == CFDEC_OUT_RGBA32F)
		hipLaunchKernelGGL((cfhip_decode_batch_kernel<FMT, TYPE, CFDEC_OUT_RGBA32F>), grid, block, 0, stream, t);
	else if (out == CFDEC_OUT_NATIVE)
		hipLaunchKernelGGL((cfhip_decode_batch_kernel<FMT, TYPE, CFDEC_OUT_NATIVE>), grid, block, 0, stream, t);
	else if constexpr ((FMT == 33 || FMT == 34) && TYPE == 0 && TB <= 2)
		hipLaunchKernelGGL((cfhip_decode_batch_kernel<FMT, TYPE, CFDEC_OUT_RGBA8>), grid, block, 0, stream, t);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

} // namespace

extern "C" hipError_t cfhip_launch_decode_batch(int format, int type, int out, const cfdec_batch_entry* table,
	uint32_t n, uint32_t total_wg, int bw, int bh, unsigned long long* errors, hipStream_t stream)
{
	cfdec_batch t;
	t.table = table;
	t.errors = errors;
	t.n = n;
	if (!n || !total_wg)
		return hipErrorInvalidValue;
	if (format >= 43 && format <= 56) {
		const dim3 grid(total_wg), block(kAstcRun);
		const bool f32 = out == CFDEC_OUT_RGBA32F;
		if (out != CFDEC_OUT_NATIVE && !f32)
			return hipErrorInvalidValue;
		if (type == 4) {
			if (f32) hipLaunchKernelGGL((cfhip_decode_batch_astc_kernel<true, CFDEC_OUT_RGBA32F>), grid, block, 0, stream, t, bw, bh);
			else hipLaunchKernelGGL((cfhip_decode_batch_astc_kernel<true, CFDEC_OUT_NATIVE>), grid, block, 0, stream, t, bw, bh);
		} else {
			if (f32) hipLaunchKernelGGL((cfhip_decode_batch_astc_kernel<false, CFDEC_OUT_RGBA32F>), grid, block, 0, stream, t, bw, bh);
			else hipLaunchKernelGGL((cfhip_decode_batch_astc_kernel<false, CFDEC_OUT_NATIVE>), grid, block, 0, stream, t, bw, bh);
		}
		return hipGetLastError();
	}
	const bool sn = type == 1;
	switch (format) {
		case 29: return launch_batch4x4<29, 0>(t, out, total_wg, stream);
		case 30: return launch_batch4x4<30, 0>(t, out, total_wg, stream);
		case 31: return launch_batch4x4<31, 0>(t, out, total_wg, stream);
		case 32: return launch_batch4x4<32, 0>(t, out, total_wg, stream);
		case 33: return sn ? launch_batch4x4<33, 1>(t, out, total_wg, stream) : launch_batch4x4<33, 0>(t, out, total_wg, stream);
		case 34: return sn ? launch_batch4x4<34, 1>(t, out, total_wg, stream) : launch_batch4x4<34, 0>(t, out, total_wg, stream);
		case 35: return type == 5 ? launch_batch4x4<35, 5>(t, out, total_wg, stream) : launch_batch4x4<35, 4>(t, out, total_wg, stream);
		case 36: return launch_batch4x4<36, 0>(t, out, total_wg, stream);
		case 37: return launch_batch4x4<37, 0>(t, out, total_wg, stream);
		case 38: return launch_batch4x4<38, 0>(t, out, total_wg, stream);
		case 39: return launch_batch4x4<39, 0>(t, out, total_wg, stream);
		case 40: return launch_batch4x4<40, 0>(t, out, total_wg, stream);
		case 41: return sn ? launch_batch4x4<41, 1>(t, out, total_wg, stream) : launch_batch4x4<41, 0>(t, out, total_wg, stream);
		case 42: return sn ? launch_batch4x4<42, 1>(t, out, total_wg, stream) : launch_batch4x4<42, 0>(t, out, total_wg, stream);
		default: return hipErrorInvalidValue;
	}
}
