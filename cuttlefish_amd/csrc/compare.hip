// compare.hip -- quality metrics of an encoded payload against a reference: SSE, log SSE, reference maximum,
// per-block error map and SSIM, every sum in FP64 and reduced in a fixed order.
//
// Shapes:
//   * Pass A, 4x4 formats: one lane per block (the decode kernels' shape).  The lane decodes its block with
//     decode4x4, normalises each texel, reads the reference texel and accumulates in FP64; the block's SSE is
//     the lane's own sum, so the error map needs no atomics.
//   * Pass A, ASTC: one wave per run of 64 blocks of a block row; phase 1 parses each block into an LDS record
//     (decode_blocks.h), phase 2 has lane b evaluate block b's texels.
//   * Pass A, standard formats: the unpack kernel's shape (std_unpack.hip): a workgroup owns 512 consecutive pixels
//     of the tight payload, a lane two of them; the pixel becomes the float the unpack kernel would store, then a
//     double.  No block grid, so no error map.
//   * Pass B (SSIM, LDR layouts): the payload is decoded into a scratch surface by the decode kernels, then one
//     256-thread workgroup per 16x16 tile of window centres stages the tile and its 5-texel halo of one channel in
//     LDS and runs the separable 11-tap Gaussian in FP64.
//   * Every workgroup writes its FP64 partials; one single-workgroup kernel reduces them in a fixed order and
//     writes the cfhip_compare_result.  No float atomics: two identical calls return identical bits.
//   * Batched launches (compare_batch.h): the per-workgroup work of every pass is a
//     __device__ function of its argument struct; the cfhip_compare_batch_* kernels resolve their surface from the
//     call's table and run the same function with the same workgroup shape, so surface i of a batch returns the
//     bits the per-surface kernels return for it alone.
// No kernel here may use scratch, spill a vector register or use AGPRs (cuttlefish_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cf_texel.h"
#include "compare_batch.h"
#include "decode_blocks.h"
#include "std_unpack.h"
#include "../../include/cuttlefish_hip.h"

namespace {

constexpr int kCmpWg = 256;       // threads of the lane-per-block, SSIM and final kernels
constexpr int kCmpRun = 64;       // ASTC blocks (and threads) of a Pass A workgroup
constexpr int kPartA = 16;        // doubles per Pass A partial: sse[4], log_sse[4], ref_max[4], error blocks, pad
constexpr int kTile = 16;         // SSIM window centres per tile side
constexpr int kHalo = 5;          // SSIM window radius
constexpr int kReg = kTile + 2*kHalo;

struct cmp_args {
	const uint8_t* blocks;
	const uint8_t* ref;
	unsigned long long ref_pitch;
	uint32_t width, height, bx, by;
	uint32_t ref_pix;             // CFHIP_PIXEL_*; ref and ref_pitch are aligned to the texel size
	uint32_t cmask;               // bit c: channel c compared
	uint32_t blk_vec;             // blocks is aligned to the block size
	float* block_errors;          // may be null
	double* partials;             // kPartA doubles per workgroup
};

__device__ __forceinline__ double half_to_double(uint32_t h)
{
	return (double)cf_half_to_float(h & 0xFFFFu);
}

__device__ __forceinline__ double snorm_div(int v, double d)
{
	const double x = (double)v/d;
	return x < -1.0 ? -1.0 : x;
}

// reference texel (x, y) as stored: RGBA8 v/255, RGBA32F and RGBA16F exactly
__device__ __forceinline__ void ref_load(const uint8_t* ref, unsigned long long pitch, uint32_t pix, uint32_t x,
	uint32_t y, double* r)
{
	const uint8_t* row = ref + (uint64_t)y*pitch;
	if (pix == CFHIP_PIXEL_RGBA8) {
		const uint32_t p = *reinterpret_cast<const uint32_t*>(row + (uint64_t)x*4u);
#pragma unroll
		for (int c = 0; c < 4; ++c)
			r[c] = (double)((p >> (8*c)) & 255u)/255.0;
	} else if (pix == CFHIP_PIXEL_RGBA32F) {
		const float4 f = *reinterpret_cast<const float4*>(row + (uint64_t)x*16u);
		r[0] = f.x; r[1] = f.y; r[2] = f.z; r[3] = f.w;
	} else {
		const uint2 h = *reinterpret_cast<const uint2*>(row + (uint64_t)x*8u);
		r[0] = half_to_double(h.x); r[1] = half_to_double(h.x >> 16);
		r[2] = half_to_double(h.y); r[3] = half_to_double(h.y >> 16);
	}
}

// texel (i, j) of a decode4x4 block, normalised; absent channels read 0
template <int FMT, int TYPE>
__device__ __forceinline__ void dec_texel(const uint32_t* w, int i, int j, double* d)
{
	constexpr int TB = texel_bytes<FMT, TYPE>();
	d[0] = d[1] = d[2] = d[3] = 0.0;
	if constexpr (FMT == 35) {
		const uint32_t lo = w[8*j + 2*i], hi = w[8*j + 2*i + 1];
		d[0] = half_to_double(lo); d[1] = half_to_double(lo >> 16);
		d[2] = half_to_double(hi); d[3] = half_to_double(hi >> 16);
	} else if constexpr (FMT == 41 || FMT == 42) {
		const uint32_t v = FMT == 41 ? (w[2*j + (i >> 1)] >> (16*(i & 1))) & 0xFFFFu : w[4*j + i];
#pragma unroll
		for (int c = 0; c < (FMT == 41 ? 1 : 2); ++c) {
			const uint32_t u = (v >> (16*c)) & 0xFFFFu;
			d[c] = TYPE == 1 ? snorm_div((int)(int16_t)u, 1023.0) : (double)u/2047.0;
		}
	} else {
		const uint32_t v = TB == 4 ? w[4*j + i] : (TB == 2 ? (w[2*j + (i >> 1)] >> (16*(i & 1))) & 0xFFFFu
			: (w[j] >> (8*i)) & 255u);
#pragma unroll
		for (int c = 0; c < TB; ++c) {
			const uint32_t u = (v >> (8*c)) & 255u;
			d[c] = TYPE == 1 ? snorm_div((int)(int8_t)u, 127.0) : (double)u/255.0;
		}
	}
}

struct Acc {
	double sse[4], lsse[4], rmax[4];
};

__device__ __forceinline__ void acc_init(Acc& s)
{
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		s.sse[c] = 0.0;
		s.lsse[c] = 0.0;
		s.rmax[c] = -__builtin_huge_val();
	}
}

// one texel into the lane's sums; returns its SSE over the compared channels
template <bool HDR>
__device__ __forceinline__ double acc_texel(Acc& s, const double* d, const double* r, uint32_t cmask)
{
	double t = 0.0;
#pragma unroll
	for (int c = 0; c < 4; ++c)
		if ((cmask >> c) & 1u) {
			const double e = d[c] - r[c];
			s.sse[c] += e*e;
			t += e*e;
			s.rmax[c] = fmax(s.rmax[c], r[c]);
			if (HDR) {
				const double tiny = 5.9604644775390625e-08;     // 2^-24
				const double l = log2(fmax(d[c], tiny)) - log2(fmax(r[c], tiny));
				s.lsse[c] += l*l;
			}
		}
	return t;
}

__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

__device__ __forceinline__ double wave_max_d(double v)
{
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1)
		v = fmax(v, __shfl_xor(v, o, 64));
	return v;
}

// the workgroup's partial (out: its kPartA doubles): per-wave butterflies, then the waves in order by thread 0
template <int NT>
__device__ __forceinline__ void write_partial(const Acc& s, double err, double* out)
{
	constexpr int NW = NT/64;
	__shared__ double wp[NW][13];
	const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		const double a = wave_sum_d(s.sse[c]), b = wave_sum_d(s.lsse[c]), m = wave_max_d(s.rmax[c]);
		if (ln == 0) { wp[wv][c] = a; wp[wv][4 + c] = b; wp[wv][8 + c] = m; }
	}
	const double e = wave_sum_d(err);
	if (ln == 0)
		wp[wv][12] = e;
	__syncthreads();
	if (threadIdx.x < 13) {
		const int q = threadIdx.x;
		double v = wp[0][q];
#pragma unroll
		for (int k = 1; k < NW; ++k)
			v = (q >= 8 && q < 12) ? fmax(v, wp[k][q]) : v + wp[k][q];
		out[q] = v;
	}
}

// Pass A of workgroup `wg` of surface a (lane-per-block formats); out: the workgroup's partial
template <int FMT, int TYPE>
__device__ __forceinline__ void compare_block_wg(const cmp_args& a, uint32_t wg, double* out)
{
	constexpr int TB = texel_bytes<FMT, TYPE>();
	constexpr int BB = (FMT == 29 || FMT == 30 || FMT == 33 || (FMT >= 37 && FMT <= 39) || FMT == 41) ? 8 : 16;
	const uint64_t b = (uint64_t)wg*kCmpWg + threadIdx.x;
	const uint64_t nblk = (uint64_t)a.bx*a.by;
	Acc s;
	acc_init(s);
	double err = 0.0;
	if (b < nblk) {
		const uint32_t by = (uint32_t)(b/a.bx), bx = (uint32_t)(b - (uint64_t)by*a.bx);
		uint64_t lo, hi;
		load_block(a.blocks + b*BB, BB, a.blk_vec != 0, lo, hi);
		uint32_t w[4*TB];
		err = decode4x4<FMT, TYPE>(lo, hi, w) ? 1.0 : 0.0;
		const uint32_t x0 = bx*4, y0 = by*4;
		double blk = 0.0;
		for (int j = 0; j < 4; ++j)
			for (int i = 0; i < 4; ++i)
				if (y0 + j < a.height && x0 + i < a.width) {
					double d[4], r[4];
					dec_texel<FMT, TYPE>(w, i, j, d);
					ref_load(a.ref, a.ref_pitch, a.ref_pix, x0 + i, y0 + j, r);
					blk += acc_texel<FMT == 35>(s, d, r, a.cmask);
				}
		if (a.block_errors)
			a.block_errors[b] = (float)blk;
	}
	write_partial<kCmpWg>(s, err, out);
}

template <int FMT, int TYPE>
__global__ __launch_bounds__(kCmpWg) void cfhip_compare_block_kernel(cmp_args a)
{
	compare_block_wg<FMT, TYPE>(a, blockIdx.x, a.partials + (uint64_t)blockIdx.x*kPartA);
}

// ---------------------------------------------------------------- batched launches (compare_batch.h)
struct cmp_batch {
	const cmp_batch_entry* table;
	uint32_t n;
	uint32_t ref_pix, cmask;
	double* partials;             // Pass A: kPartA doubles per workgroup of the call
};

// entry of Pass A workgroup wg: a wave-uniform binary search over wg_begin (cf_resolve's, cf_device.h)
__device__ __forceinline__ uint32_t batch_surface(const cmp_batch& t, uint32_t wg, cmp_args& a, uint32_t& wgx)
{
	uint32_t lo = 0, hi = t.n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1u) >> 1;
		if (t.table[mid].wg_begin <= wg) lo = mid; else hi = mid - 1u;
	}
	const cmp_batch_entry e = t.table[lo];
	a.blocks = e.blocks; a.ref = e.ref; a.ref_pitch = e.ref_pitch;
	a.width = e.width; a.height = e.height; a.bx = e.bx; a.by = e.by;
	a.ref_pix = t.ref_pix; a.cmask = t.cmask; a.blk_vec = e.blk_vec;
	a.block_errors = e.block_errors;
	a.partials = t.partials;
	wgx = e.wgx;
	return wg - e.wg_begin;
}

template <int FMT, int TYPE>
__global__ __launch_bounds__(kCmpWg) void cfhip_compare_batch_block_kernel(cmp_batch t)
{
	cmp_args a;
	uint32_t wgx;
	const uint32_t local = batch_surface(t, blockIdx.x, a, wgx);
	compare_block_wg<FMT, TYPE>(a, local, t.partials + (uint64_t)blockIdx.x*kPartA);
}

struct std_cmp_args {
	const uint8_t* pixels;        // the tight payload, any alignment
	const uint8_t* ref;
	unsigned long long ref_pitch;
	uint32_t width, height;
	uint32_t format, type;
	uint32_t in_vec;              // pixels is aligned for the vector load of its pixel size
	uint32_t ref_pix, cmask;
	uint32_t hdr;                 // Float / UFloat types: log_sse is accumulated
	double* partials;             // kPartA doubles per workgroup
};

// Pass A for the standard formats: BPP bytes per pixel, one workgroup per cfstd::kPixPerWg pixels
template <int BPP>
__global__ __launch_bounds__(kCmpWg) void cfhip_std_compare_kernel(std_cmp_args a)
{
	static_assert(cfstd::kThreads == kCmpWg, "write_partial reduces kCmpWg threads");
	__shared__ uint32_t stage[cfstd::stage_dwords<BPP>()];
	const unsigned long long npix = (unsigned long long)a.width*a.height;
	const unsigned long long p0 = (unsigned long long)blockIdx.x*cfstd::kPixPerWg;
	uint4 o[cfstd::kPerThread];
	cfstd::load_pixels<BPP>(a.pixels, a.in_vec, p0, npix, threadIdx.x, stage, o);
	Acc s;
	acc_init(s);
#pragma unroll
	for (uint32_t j = 0; j < cfstd::kPerThread; ++j) {
		const unsigned long long p = p0 + j*cfstd::kThreads + threadIdx.x;
		if (p >= npix)
			continue;
		const uint32_t y = (uint32_t)(p/a.width), x = (uint32_t)(p - (unsigned long long)y*a.width);
		const float4 f = cfstd::unpack_pixel<BPP>(a.format, a.type, o[j]);
		const double d[4] = {(double)f.x, (double)f.y, (double)f.z, (double)f.w};
		double r[4];
		ref_load(a.ref, a.ref_pitch, a.ref_pix, x, y, r);
		if (a.hdr)
			acc_texel<true>(s, d, r, a.cmask);
		else
			acc_texel<false>(s, d, r, a.cmask);
	}
	write_partial<kCmpWg>(s, 0.0, a.partials + (uint64_t)blockIdx.x*kPartA);
}

// one wave = a run of kCmpRun blocks of one block row; grid (ceil(bx / kCmpRun), by)
// (run: the run's index in its block row; out: the workgroup's partial)
template <bool HDR>
__device__ __forceinline__ void compare_astc_wg(const cmp_args& a, int bw, int bh, uint32_t run, uint32_t by, double* out)
{
	__shared__ AstcRec rec[kCmpRun];
	const uint32_t run0 = run*kCmpRun;
	const uint32_t nb = a.bx - run0 < (uint32_t)kCmpRun ? a.bx - run0 : (uint32_t)kCmpRun;
	const uint64_t b = (uint64_t)by*a.bx + run0 + threadIdx.x;
	if (threadIdx.x < nb) {
		uint64_t lo, hi;
		load_block(a.blocks + b*16u, 16, a.blk_vec != 0, lo, hi);
		astc_parse(lo, hi, bw, bh, HDR, rec[threadIdx.x]);
	}
	__syncthreads();
	Acc s;
	acc_init(s);
	double err = 0.0;
	if (threadIdx.x < nb) {
		const AstcRec& r = rec[threadIdx.x];
		err = (r.status < 0 || r.bad) ? 1.0 : 0.0;
		const uint32_t x0 = (run0 + threadIdx.x)*bw, y0 = by*bh;
		const int nw = a.width - x0 < (uint32_t)bw ? (int)(a.width - x0) : bw;
		const int nh = a.height - y0 < (uint32_t)bh ? (int)(a.height - y0) : bh;
		double blk = 0.0;
		for (int t = 0; t < nh; ++t)
			for (int u = 0; u < nw; ++u) {
				uint32_t o[2];
				astc_texel<HDR>(r, bw, bh, u, t, o);
				double d[4], rf[4];
				if (HDR) {
					d[0] = half_to_double(o[0]); d[1] = half_to_double(o[0] >> 16);
					d[2] = half_to_double(o[1]); d[3] = half_to_double(o[1] >> 16);
				} else {
#pragma unroll
					for (int c = 0; c < 4; ++c)
						d[c] = (double)((o[0] >> (8*c)) & 255u)/255.0;
				}
				ref_load(a.ref, a.ref_pitch, a.ref_pix, x0 + u, y0 + t, rf);
				blk += acc_texel<HDR>(s, d, rf, a.cmask);
			}
		if (a.block_errors)
			a.block_errors[b] = (float)blk;
	}
	// one wave per workgroup
	Acc t = s;
	double e = wave_sum_d(err);
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		t.sse[c] = wave_sum_d(s.sse[c]);
		t.lsse[c] = wave_sum_d(s.lsse[c]);
		t.rmax[c] = wave_max_d(s.rmax[c]);
	}
	if (threadIdx.x < 13) {
		const int q = threadIdx.x;
		double v = e;
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			if (q == c) v = t.sse[c];
			if (q == 4 + c) v = t.lsse[c];
			if (q == 8 + c) v = t.rmax[c];
		}
		out[q] = v;
	}
}

// the partial's index is the workgroup's linear index
template <bool HDR>
__global__ __launch_bounds__(kCmpRun) void cfhip_compare_astc_kernel(cmp_args a, int bw, int bh)
{
	compare_astc_wg<HDR>(a, bw, bh, blockIdx.x, blockIdx.y, a.partials + ((uint64_t)blockIdx.y*gridDim.x + blockIdx.x)*kPartA);
}

template <bool HDR>
__global__ __launch_bounds__(kCmpRun) void cfhip_compare_batch_astc_kernel(cmp_batch t, int bw, int bh)
{
	cmp_args a;
	uint32_t wgx;
	const uint32_t local = batch_surface(t, blockIdx.x, a, wgx);
	const uint32_t by = local/wgx;
	compare_astc_wg<HDR>(a, bw, bh, local - by*wgx, by, t.partials + (uint64_t)blockIdx.x*kPartA);
}

// ---------------------------------------------------------------- Pass B: SSIM on the decoded surface

struct ssim_args {
	const uint8_t* dec;           // decoded layout, dec_pitch bytes between rows
	const uint8_t* ref;
	unsigned long long dec_pitch, ref_pitch;
	uint32_t width, height, tiles_x;
	uint32_t layout, ref_pix, cmask;
	float w[11];                  // the normalised Gaussian taps, rounded to float on the host
	double c1, c2;
	double* partials;             // 4 doubles per workgroup
};

// channel c of decoded texel (x, y), normalised; LDR layouts, and the unpacked texels of a UNorm / SNorm standard format
__device__ __forceinline__ double dec_channel(const ssim_args& a, uint32_t x, uint32_t y, int c)
{
	const uint8_t* row = a.dec + (uint64_t)y*a.dec_pitch;
	switch (a.layout) {
		case CFHIP_LAYOUT_RGBA8: return (double)row[(uint64_t)x*4u + c]/255.0;
		case CFHIP_LAYOUT_R8: return (double)row[x]/255.0;
		case CFHIP_LAYOUT_R8_SNORM: return snorm_div((int)(int8_t)row[x], 127.0);
		case CFHIP_LAYOUT_RG8: return (double)row[(uint64_t)x*2u + c]/255.0;
		case CFHIP_LAYOUT_RG8_SNORM: return snorm_div((int)(int8_t)row[(uint64_t)x*2u + c], 127.0);
		case CFHIP_LAYOUT_RGBA32F: return (double)reinterpret_cast<const float*>(row)[(uint64_t)x*4u + c];
		default: break;
	}
	const uint64_t o = (uint64_t)x*(a.layout >= CFHIP_LAYOUT_RG16 ? 4u : 2u) + 2u*c;
	const uint32_t u = (uint32_t)row[o] | ((uint32_t)row[o + 1] << 8);
	if (a.layout == CFHIP_LAYOUT_R16 || a.layout == CFHIP_LAYOUT_RG16)
		return (double)u/2047.0;
	return snorm_div((int)(int16_t)u, 1023.0);
}

__device__ __forceinline__ double ref_channel(const ssim_args& a, uint32_t x, uint32_t y, int c)
{
	const uint8_t* row = a.ref + (uint64_t)y*a.ref_pitch;
	if (a.ref_pix == CFHIP_PIXEL_RGBA8)
		return (double)row[(uint64_t)x*4u + c]/255.0;
	if (a.ref_pix == CFHIP_PIXEL_RGBA32F)
		return (double)reinterpret_cast<const float*>(row)[(uint64_t)x*4u + c];
	return half_to_double(reinterpret_cast<const uint16_t*>(row)[(uint64_t)x*4u + c]);
}

// one workgroup per kTile x kTile window centres: tile (tx, ty), centre (5 + tx*16 + lx, 5 + ty*16 + ly); out: the
// tile's 4 doubles
__device__ __forceinline__ void ssim_tile(const ssim_args& a, uint32_t tx, uint32_t ty, double* out)
{
	__shared__ double xs[kReg][kReg], ys[kReg][kReg];
	__shared__ double hs[5][kReg][kTile];
	const uint32_t ox = tx*kTile, oy = ty*kTile;
	const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
	const uint32_t cx = ox + kHalo + lx, cy = oy + kHalo + ly;
	const bool valid = cx + kHalo < a.width && cy + kHalo < a.height;
	double acc[4] = {0.0, 0.0, 0.0, 0.0};
	for (int c = 0; c < 4; ++c) {
		if (!((a.cmask >> c) & 1u))
			continue;
		__syncthreads();
		for (int k = threadIdx.x; k < kReg*kReg; k += kCmpWg) {
			const int ry = k / kReg, rx = k - ry*kReg;
			const uint32_t x = ox + rx, y = oy + ry;
			const bool in = x < a.width && y < a.height;
			xs[ry][rx] = in ? dec_channel(a, x, y, c) : 0.0;
			ys[ry][rx] = in ? ref_channel(a, x, y, c) : 0.0;
		}
		__syncthreads();
		for (int k = threadIdx.x; k < kReg*kTile; k += kCmpWg) {
			const int ry = k / kTile, col = k - ry*kTile;
			double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
			for (int t = 0; t < 11; ++t) {
				const double w = (double)a.w[t], x = xs[ry][col + t], y = ys[ry][col + t];
				sx += w*x; sy += w*y; sxx += w*(x*x); syy += w*(y*y); sxy += w*(x*y);
			}
			hs[0][ry][col] = sx; hs[1][ry][col] = sy; hs[2][ry][col] = sxx; hs[3][ry][col] = syy;
			hs[4][ry][col] = sxy;
		}
		__syncthreads();
		double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
		for (int t = 0; t < 11; ++t) {
			const double w = (double)a.w[t];
#pragma unroll
			for (int q = 0; q < 5; ++q)
				m[q] += w*hs[q][ly + t][lx];
		}
		const double mx = m[0], my = m[1];
		const double vx = m[2] - mx*mx, vy = m[3] - my*my, cxy = m[4] - mx*my;
		const double ssim = ((2.0*mx*my + a.c1)*(2.0*cxy + a.c2))/((mx*mx + my*my + a.c1)*(vx + vy + a.c2));
		if (valid)
			acc[c] = ssim;
	}
	__shared__ double wp[kCmpWg/64][4];
	const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
	for (int c = 0; c < 4; ++c) {
		const double v = wave_sum_d(acc[c]);
		if (ln == 0)
			wp[wv][c] = v;
	}
	__syncthreads();
	if (threadIdx.x < 4) {
		const int c = threadIdx.x;
		const double v = ((wp[0][c] + wp[1][c]) + wp[2][c]) + wp[3][c];
		out[c] = v;
	}
}

// grid (tiles_x, tiles_y)
__global__ __launch_bounds__(kCmpWg) void cfhip_compare_ssim_kernel(ssim_args a)
{
	ssim_tile(a, blockIdx.x, blockIdx.y, a.partials + ((uint64_t)blockIdx.y*a.tiles_x + blockIdx.x)*4u);
}

struct ssim_batch {
	const cmp_batch_entry* table;
	uint32_t n;
	uint32_t layout, ref_pix, cmask, texel_bytes;
	const uint8_t* scratch;       // the decoded surfaces, entry i at dec_off
	float w[11];
	double c1, c2;
	double* partials;             // 4 doubles per tile of the call
};

// 1-D grid over the tiles of the call; surfaces without a valid window own no tile and are never found
__global__ __launch_bounds__(kCmpWg) void cfhip_compare_batch_ssim_kernel(ssim_batch t)
{
	const uint32_t tile = blockIdx.x;
	uint32_t lo = 0, hi = t.n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1u) >> 1;
		if (t.table[mid].tile_begin <= tile) lo = mid; else hi = mid - 1u;
	}
	const cmp_batch_entry e = t.table[lo];
	ssim_args a;
	a.dec = t.scratch + e.dec_off;
	a.ref = e.ref;
	a.dec_pitch = (unsigned long long)e.width*t.texel_bytes;
	a.ref_pitch = e.ref_pitch;
	a.width = e.width; a.height = e.height; a.tiles_x = e.tiles_x;
	a.layout = t.layout; a.ref_pix = t.ref_pix; a.cmask = t.cmask;
#pragma unroll
	for (int k = 0; k < 11; ++k)
		a.w[k] = t.w[k];
	a.c1 = t.c1; a.c2 = t.c2;
	a.partials = t.partials;
	const uint32_t local = tile - e.tile_begin, ty = local/e.tiles_x;
	ssim_tile(a, local - ty*e.tiles_x, ty, t.partials + (uint64_t)tile*4u);
}

// ---------------------------------------------------------------- the final reduction

struct final_args {
	const double* pa;             // Pass A partials, na x kPartA
	const double* pb;             // SSIM partials, nb x 4 (null: SSIM not computed)
	uint64_t na, nb;
	uint64_t texels;
	uint32_t cmask, hdr, windows;
	cfhip_compare_result* result;
};

// one workgroup: thread t folds rows t, t + 256, ... in order, then column q is folded over the threads in order
__device__ __forceinline__ void final_fold(const final_args& f)
{
	constexpr int NQ = 17;        // 13 Pass A fields, 4 SSIM sums
	__shared__ double part[NQ][kCmpWg];
	double v[NQ];
#pragma unroll
	for (int q = 0; q < NQ; ++q)
		v[q] = (q >= 8 && q < 12) ? -__builtin_huge_val() : 0.0;
	for (uint64_t i = threadIdx.x; i < f.na; i += kCmpWg) {
		const double* p = f.pa + i*kPartA;
#pragma unroll
		for (int q = 0; q < 13; ++q)
			v[q] = (q >= 8 && q < 12) ? fmax(v[q], p[q]) : v[q] + p[q];
	}
	if (f.pb)
		for (uint64_t i = threadIdx.x; i < f.nb; i += kCmpWg) {
#pragma unroll
			for (int c = 0; c < 4; ++c)
				v[13 + c] += f.pb[i*4u + c];
		}
#pragma unroll
	for (int q = 0; q < NQ; ++q)
		part[q][threadIdx.x] = v[q];
	__syncthreads();
	if (threadIdx.x < NQ) {
		const int q = threadIdx.x;
		double s = part[q][0];
		for (int t = 1; t < kCmpWg; ++t)
			s = (q >= 8 && q < 12) ? fmax(s, part[q][t]) : s + part[q][t];
		part[q][0] = s;
	}
	__syncthreads();
	if (threadIdx.x >= 4)
		return;
	const int c = threadIdx.x;
	const double nan = __builtin_nan("");
	const bool on = (f.cmask >> c) & 1u;
	cfhip_compare_result* r = f.result;
	r->sse[c] = on ? part[c][0] : 0.0;
	r->log_sse[c] = on ? (f.hdr ? part[4 + c][0] : nan) : 0.0;
	r->ref_max[c] = on ? part[8 + c][0] : 0.0;
	r->ssim[c] = (on && f.pb && f.windows) ? part[13 + c][0]/(double)f.windows : nan;
	if (c == 0) {
		r->texels = f.texels;
		r->error_blocks = (uint64_t)part[12][0];
		r->channels = f.cmask;
		r->ssim_windows = f.pb ? f.windows : 0u;
	}
}

__global__ __launch_bounds__(kCmpWg) void cfhip_compare_final_kernel(final_args f)
{
	final_fold(f);
}

struct final_batch {
	const cmp_batch_entry* table;
	const double* pa;             // Pass A partials of the call
	const double* pb;             // SSIM partials of the call (null: no SSIM pass)
	uint32_t cmask, hdr;
	cfhip_compare_result* results;
};

// workgroup i folds surface i's partials, in cfhip_compare_final_kernel's order
__global__ __launch_bounds__(kCmpWg) void cfhip_compare_batch_final_kernel(final_batch t)
{
	const cmp_batch_entry e = t.table[blockIdx.x];
	final_args f;
	f.pa = t.pa + (uint64_t)e.wg_begin*kPartA;
	// a surface without tiles folds as a per-surface call without the SSIM flag does: NaN, 0 windows
	f.pb = (t.pb && e.nb) ? t.pb + (uint64_t)e.tile_begin*4u : nullptr;
	f.na = e.na; f.nb = e.nb;
	f.texels = (uint64_t)e.width*e.height;
	f.cmask = t.cmask; f.hdr = t.hdr;
	f.windows = e.windows;
	f.result = t.results + blockIdx.x;
	final_fold(f);
}

template <int FMT, int TYPE>
hipError_t launch_a(const cmp_args& a, hipStream_t stream)
{
	const uint64_t nblk = (uint64_t)a.bx*a.by;
	hipLaunchKernelGGL((cfhip_compare_block_kernel<FMT, TYPE>), dim3((uint32_t)((nblk + kCmpWg - 1)/kCmpWg)),
		dim3(kCmpWg), 0, stream, a);
	return hipGetLastError();
}

} // namespace

// Workgroups (and so partials) of Pass A and of the SSIM pass for a surface; cfhip_api.hip sizes its scratch with
// these.  SSIM: 0 when a side is below 11 (no valid window centre).
extern "C" uint64_t cfhip_compare_partials(int format, uint32_t width, uint32_t height, uint32_t bx, uint32_t by,
	uint64_t* ssim_partials)
{
	if (ssim_partials) {
		*ssim_partials = (width < 11 || height < 11) ? 0 :
			(uint64_t)((width - 10 + kTile - 1)/kTile)*((height - 10 + kTile - 1)/kTile);
	}
	if (format >= 43 && format <= 56)
		return (uint64_t)((bx + kCmpRun - 1)/kCmpRun)*by;
	return ((uint64_t)bx*by + kCmpWg - 1)/kCmpWg;
}

// Host launchers (cfhip_api.hip checks every argument first).
// Pass A: partials receives cfhip_compare_partials() x 16 doubles; block_errors (may be null) bx*by floats.
extern "C" hipError_t cfhip_launch_compare(int format, int type, const void* blocks, int blk_vec, const void* ref,
	int ref_pix, size_t ref_pitch, uint32_t width, uint32_t height, uint32_t bx, uint32_t by, int bw, int bh,
	unsigned cmask, float* block_errors, double* partials, hipStream_t stream)
{
	cmp_args a;
	a.blocks = static_cast<const uint8_t*>(blocks);
	a.ref = static_cast<const uint8_t*>(ref);
	a.ref_pitch = ref_pitch;
	a.width = width; a.height = height; a.bx = bx; a.by = by;
	a.ref_pix = (uint32_t)ref_pix;
	a.cmask = cmask;
	a.blk_vec = (uint32_t)blk_vec;
	a.block_errors = block_errors;
	a.partials = partials;
	if (format >= 43 && format <= 56) {
		const dim3 grid((bx + kCmpRun - 1)/kCmpRun, by), block(kCmpRun);
		if (type == 4)
			hipLaunchKernelGGL(cfhip_compare_astc_kernel<true>, grid, block, 0, stream, a, bw, bh);
		else
			hipLaunchKernelGGL(cfhip_compare_astc_kernel<false>, grid, block, 0, stream, a, bw, bh);
		return hipGetLastError();
	}
	const bool sn = type == 1;
	switch (format) {
		case 29: return launch_a<29, 0>(a, stream);
		case 30: return launch_a<30, 0>(a, stream);
		case 31: return launch_a<31, 0>(a, stream);
		case 32: return launch_a<32, 0>(a, stream);
		case 33: return sn ? launch_a<33, 1>(a, stream) : launch_a<33, 0>(a, stream);
		case 34: return sn ? launch_a<34, 1>(a, stream) : launch_a<34, 0>(a, stream);
		case 35: return type == 5 ? launch_a<35, 5>(a, stream) : launch_a<35, 4>(a, stream);
		case 36: return launch_a<36, 0>(a, stream);
		case 37: return launch_a<37, 0>(a, stream);
		case 38: return launch_a<38, 0>(a, stream);
		case 39: return launch_a<39, 0>(a, stream);
		case 40: return launch_a<40, 0>(a, stream);
		case 41: return sn ? launch_a<41, 1>(a, stream) : launch_a<41, 0>(a, stream);
		case 42: return sn ? launch_a<42, 1>(a, stream) : launch_a<42, 0>(a, stream);
		default: return hipErrorInvalidValue;
	}
}

// Workgroups (partials) of the standard formats' Pass A; the SSIM pass's as above.
extern "C" uint64_t cfhip_std_compare_partials(uint32_t width, uint32_t height, uint64_t* ssim_partials)
{
	if (ssim_partials)
		cfhip_compare_partials(0, width, height, 0, 0, ssim_partials);
	return ((uint64_t)width*height + cfstd::kPixPerWg - 1)/cfstd::kPixPerWg;
}

// Pass A for a legal standard (format, type) pair of bytes_per_pixel bytes; partials receives
// cfhip_std_compare_partials() x 16 doubles.
extern "C" hipError_t cfhip_launch_std_compare(int format, int type, int bytes_per_pixel, const void* pixels,
	const void* ref, int ref_pix, size_t ref_pitch, uint32_t width, uint32_t height, unsigned cmask, int hdr,
	double* partials, hipStream_t stream)
{
	std_cmp_args a;
	a.pixels = static_cast<const uint8_t*>(pixels);
	a.ref = static_cast<const uint8_t*>(ref);
	a.ref_pitch = ref_pitch;
	a.width = width; a.height = height;
	a.format = (uint32_t)format; a.type = (uint32_t)type;
	const uintptr_t al = bytes_per_pixel == 16 ? 16u : (bytes_per_pixel == 8 ? 8u : 4u);
	a.in_vec = (uintptr_t)pixels % al == 0 ? 1u : 0u;
	a.ref_pix = (uint32_t)ref_pix;
	a.cmask = cmask;
	a.hdr = (uint32_t)hdr;
	a.partials = partials;
	const dim3 grid((unsigned)cfhip_std_compare_partials(width, height, nullptr)), block(kCmpWg);
	switch (bytes_per_pixel) {
		case 1: hipLaunchKernelGGL(cfhip_std_compare_kernel<1>, grid, block, 0, stream, a); break;
		case 2: hipLaunchKernelGGL(cfhip_std_compare_kernel<2>, grid, block, 0, stream, a); break;
		case 3: hipLaunchKernelGGL(cfhip_std_compare_kernel<3>, grid, block, 0, stream, a); break;
		case 4: hipLaunchKernelGGL(cfhip_std_compare_kernel<4>, grid, block, 0, stream, a); break;
		case 6: hipLaunchKernelGGL(cfhip_std_compare_kernel<6>, grid, block, 0, stream, a); break;
		case 8: hipLaunchKernelGGL(cfhip_std_compare_kernel<8>, grid, block, 0, stream, a); break;
		case 12: hipLaunchKernelGGL(cfhip_std_compare_kernel<12>, grid, block, 0, stream, a); break;
		case 16: hipLaunchKernelGGL(cfhip_std_compare_kernel<16>, grid, block, 0, stream, a); break;
		default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

// Pass B over a decoded surface (LDR layouts); taps: the 11 normalised Gaussian weights; range: L of C1, C2.
extern "C" hipError_t cfhip_launch_ssim(const void* dec, size_t dec_pitch, int layout, const void* ref, int ref_pix,
	size_t ref_pitch, uint32_t width, uint32_t height, unsigned cmask, const float* taps, double range,
	double* partials, hipStream_t stream)
{
	ssim_args a;
	a.dec = static_cast<const uint8_t*>(dec);
	a.ref = static_cast<const uint8_t*>(ref);
	a.dec_pitch = dec_pitch;
	a.ref_pitch = ref_pitch;
	a.width = width; a.height = height;
	a.tiles_x = (width - 10 + kTile - 1)/kTile;
	a.layout = (uint32_t)layout;
	a.ref_pix = (uint32_t)ref_pix;
	a.cmask = cmask;
	for (int t = 0; t < 11; ++t)
		a.w[t] = taps[t];
	a.c1 = (0.01*range)*(0.01*range);
	a.c2 = (0.03*range)*(0.03*range);
	a.partials = partials;
	const dim3 grid(a.tiles_x, (height - 10 + kTile - 1)/kTile);
	hipLaunchKernelGGL(cfhip_compare_ssim_kernel, grid, dim3(kCmpWg), 0, stream, a);
	return hipGetLastError();
}

// The final reduction into *result (device memory); pb null: SSIM not computed.
extern "C" hipError_t cfhip_launch_compare_final(const double* pa, uint64_t na, const double* pb, uint64_t nb,
	unsigned cmask, int hdr, uint32_t windows, uint64_t texels, cfhip_compare_result* result, hipStream_t stream)
{
	final_args f;
	f.pa = pa; f.pb = pb; f.na = na; f.nb = nb;
	f.texels = texels;
	f.cmask = cmask;
	f.hdr = (uint32_t)hdr;
	f.windows = windows;
	f.result = result;
	hipLaunchKernelGGL(cfhip_compare_final_kernel, dim3(1), dim3(kCmpWg), 0, stream, f);
	return hipGetLastError();
}

// ---------------------------------------------------------------- batched launchers (compare_batch.h)
namespace {

template <int FMT, int TYPE>
hipError_t launch_batch_a(const cmp_batch& t, uint32_t total_wg, hipStream_t stream)
{
	hipLaunchKernelGGL((cfhip_compare_batch_block_kernel<FMT, TYPE>), dim3(total_wg), dim3(kCmpWg), 0, stream, t);
	return hipGetLastError();
}

} // namespace

extern "C" hipError_t cfhip_launch_compare_batch(int format, int type, const cmp_batch_entry* table, uint32_t n,
	uint32_t total_wg, int bw, int bh, int ref_pix, unsigned cmask, double* partials, hipStream_t stream)
{
	if (!n || !total_wg)
		return hipErrorInvalidValue;
	cmp_batch t;
	t.table = table;
	t.n = n;
	t.ref_pix = (uint32_t)ref_pix;
	t.cmask = cmask;
	t.partials = partials;
	if (format >= 43 && format <= 56) {
		const dim3 grid(total_wg), block(kCmpRun);
		if (type == 4)
			hipLaunchKernelGGL(cfhip_compare_batch_astc_kernel<true>, grid, block, 0, stream, t, bw, bh);
		else
			hipLaunchKernelGGL(cfhip_compare_batch_astc_kernel<false>, grid, block, 0, stream, t, bw, bh);
		return hipGetLastError();
	}
	const bool sn = type == 1;
	switch (format) {
		case 29: return launch_batch_a<29, 0>(t, total_wg, stream);
		case 30: return launch_batch_a<30, 0>(t, total_wg, stream);
		case 31: return launch_batch_a<31, 0>(t, total_wg, stream);
		case 32: return launch_batch_a<32, 0>(t, total_wg, stream);
		case 33: return sn ? launch_batch_a<33, 1>(t, total_wg, stream) : launch_batch_a<33, 0>(t, total_wg, stream);
		case 34: return sn ? launch_batch_a<34, 1>(t, total_wg, stream) : launch_batch_a<34, 0>(t, total_wg, stream);
		case 35: return type == 5 ? launch_batch_a<35, 5>(t, total_wg, stream) : launch_batch_a<35, 4>(t, total_wg, stream);
		case 36: return launch_batch_a<36, 0>(t, total_wg, stream);
		case 37: return launch_batch_a<37, 0>(t, total_wg, stream);
		case 38: return launch_batch_a<38, 0>(t, total_wg, stream);
		case 39: return launch_batch_a<39, 0>(t, total_wg, stream);
		case 40: return launch_batch_a<40, 0>(t, total_wg, stream);
		case 41: return sn ? launch_batch_a<41, 1>(t, total_wg, stream) : launch_batch_a<41, 0>(t, total_wg, stream);
		case 42: return sn ? launch_batch_a<42, 1>(t, total_wg, stream) : launch_batch_a<42, 0>(t, total_wg, stream);
		default: return hipErrorInvalidValue;
	}
}

extern "C" hipError_t cfhip_launch_ssim_batch(const cmp_batch_entry* table, uint32_t n, uint32_t total_tiles,
	const void* scratch, int layout, int ref_pix, unsigned cmask, const float* taps, double range, double* partials,
	hipStream_t stream)
{
	if (!n || !total_tiles)
		return hipErrorInvalidValue;
	ssim_batch t;
	t.table = table;
	t.n = n;
	t.layout = (uint32_t)layout;
	t.ref_pix = (uint32_t)ref_pix;
	t.cmask = cmask;
	switch (layout) {
		case CFHIP_LAYOUT_R8: case CFHIP_LAYOUT_R8_SNORM: t.texel_bytes = 1; break;
		case CFHIP_LAYOUT_RG8: case CFHIP_LAYOUT_RG8_SNORM: case CFHIP_LAYOUT_R16: case CFHIP_LAYOUT_R16_SNORM:
			t.texel_bytes = 2; break;
		case CFHIP_LAYOUT_RGBA8: case CFHIP_LAYOUT_RG16: case CFHIP_LAYOUT_RG16_SNORM: t.texel_bytes = 4; break;
		default: return hipErrorInvalidValue;      // HDR layouts have no SSIM pass
	}
	t.scratch = static_cast<const uint8_t*>(scratch);
	for (int k = 0; k < 11; ++k)
		t.w[k] = taps[k];
	t.c1 = (0.01*range)*(0.01*range);
	t.c2 = (0.03*range)*(0.03*range);
	t.partials = partials;
	hipLaunchKernelGGL(cfhip_compare_batch_ssim_kernel, dim3(total_tiles), dim3(kCmpWg), 0, stream, t);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_compare_batch_final(const cmp_batch_entry* table, uint32_t n, const double* pa,
	const double* pb, unsigned cmask, int hdr, cfhip_compare_result* results, hipStream_t stream)
{
	if (!n)
		return hipErrorInvalidValue;
	final_batch t;
	t.table = table;
	t.pa = pa; t.pb = pb;
	t.cmask = cmask;
	t.hdr = (uint32_t)hdr;
	t.results = results;
	hipLaunchKernelGGL(cfhip_compare_batch_final_kernel, dim3(n), dim3(kCmpWg), 0, stream, t);
	return hipGetLastError();
}
