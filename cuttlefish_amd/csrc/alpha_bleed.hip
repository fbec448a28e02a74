// alpha_bleed.hip -- alpha bleeding: every texel whose alpha is not above a threshold takes
// the R, G, B storage bits of the nearest texel whose alpha is, so that filters and block encoders see a sensible colour
// on both sides of a cut-out's silhouette.  Alpha is untouched.
//
// The nearest seed is found by a jump flood over seed words (x | y << 16, CFAB_NONE for none) in two ping-pong buffers:
// pass 0 writes each texel's own word, then steps P/2 ... 1 and one more 1 (P the power of two at or above the larger
// side) each keep, per texel, the seed of minimal key d^2 << 32 | word among the nine stored at p + step * {-1, 0, 1}^2.
// The key orders ties, so the result does not depend on the order of the reads (include/cuttlefish_hip.h has the
// definition in full; tests/alpha_bleed_ref.py restates it in numpy).
//
//   seed  alpha read once per texel, its word written, the seeds counted.  A wavefront walks CFAB_ROWS rows, four
//         apart, and the four wavefronts of a workgroup add up in LDS before one vector atomic goes to memory: with
//         one atomic per 64 texels the counter's one address, not the memory, set the pass's time (1.9 ms of a
//         4096^2 surface, the fill 6 ms)
//   step  nine gathers per texel; a wavefront is 64 texels of one row, so each gather of a wavefront is one contiguous
//         row segment of the buffer
//   fill  the last step, not written back: a texel that is no seed and found one within max_distance copies the seed
//         texel's colour components as stored.  Seed texels are never written and only seed texels are read, so the
//         pass is in place.  filled and max d^2 are reduced over the wavefront, then over the workgroup in LDS: one
//         vector atomic each per workgroup of 64 x 64 texels.
// All layers of a call share every launch (grid z).  No kernel here may use scratch, spill a vector register or use
// AGPRs (cuttlefish_amd/build.py).
#include "cf_texel.h"
#include "alpha_bleed.h"

namespace {

constexpr uint32_t WG = CFAB_WG_X*CFAB_WG_Y;

// the minimal key among the seeds stored at (x, y) + {-1, 0, 1}^2 * (kx, ky), ~0 if there is none.  All nine loads
// are issued before any is used.  A position outside an unwrapped axis is replaced by the texel's own on that axis:
// that is another of the nine candidates, so the minimum does not change and no candidate carries a validity flag
// (the steps are bound by vector instructions, not by memory: DESIGN.md section 4.21).  kx < width on a wrapped x axis
// (the step modulo the size), the same for y.  WRAP: some axis wraps; without, the distance needs no absolute value.
template <bool WRAP>
__device__ __forceinline__ uint64_t nearest(const cfab_call& c, const uint32_t* __restrict__ in, uint32_t x, uint32_t y,
	uint32_t kx, uint32_t ky)
{
	const uint32_t w = c.width, h = c.height;
	const bool wx = WRAP && (c.flags & CFHIP_BLEED_WRAP_X), wy = WRAP && (c.flags & CFHIP_BLEED_WRAP_Y);
	uint32_t xs[3], ys[3];
	xs[1] = x;
	xs[0] = x >= kx ? x - kx : wx ? x + w - kx : x;
	xs[2] = x + kx < w ? x + kx : wx ? x + kx - w : x;
	ys[1] = y;
	ys[0] = y >= ky ? y - ky : wy ? y + h - ky : y;
	ys[2] = y + ky < h ? y + ky : wy ? y + ky - h : y;
	uint32_t s[9];
#pragma unroll
	for (int j = 0; j < 3; ++j)
#pragma unroll
		for (int i = 0; i < 3; ++i)
			s[j*3 + i] = in[ys[j]*w + xs[i]];
	uint64_t best = ~0ull;
#pragma unroll
	for (int i = 0; i < 9; ++i) {
		const uint32_t v = s[i];
		int32_t dx = (int32_t)x - (int32_t)(v & 0xFFFFu), dy = (int32_t)y - (int32_t)(v >> 16);
		if (wx) {
			dx = abs(dx);
			dx = min(dx, (int32_t)w - dx);
		}
		if (wy) {
			dy = abs(dy);
			dy = min(dy, (int32_t)h - dy);
		}
		// (|dx|, |dy| < 2^16, also for the word of no seed: the full-rate 24-bit multiply is exact)
		const uint32_t d2 = v == CFAB_NONE ? ~0u : (uint32_t)(__mul24(dx, dx) + __mul24(dy, dy));
		const uint64_t key = (uint64_t)d2 << 32 | v;
		best = key < best ? key : best;
	}
	return best;
}

__global__ void __launch_bounds__(WG)
cfhip_alpha_bleed_seed_kernel(cfab_call c, float t, uint32_t* __restrict__ seeds, cfhip_bleed_result* __restrict__ results)
{
	__shared__ float of_u8[256];
	__shared__ uint32_t sum;                           // the workgroup's seeds: its wavefronts meet here before memory
	const uint32_t v = threadIdx.y*CFAB_WG_X + threadIdx.x;
	cf_fill_of_u8(of_u8, v, c.pixel_type == CFHIP_PIXEL_RGBA8);
	if (v == 0)
		sum = 0;
	__syncthreads();
	const uint32_t x = blockIdx.x*CFAB_WG_X + threadIdx.x, layer = blockIdx.z;
	const bool active = x < c.width;
	uint32_t n = 0;
	for (uint32_t j = 0; j < CFAB_ROWS; ++j) {
		const uint32_t y = (blockIdx.y*CFAB_ROWS + j)*CFAB_WG_Y + threadIdx.y;
		if (y >= c.height)
			break;                                     // the whole wavefront: it shares y
		float a = __builtin_nanf("");                  // a texel outside the surface is no seed
		if (active) {
			const uint8_t* row = static_cast<const uint8_t*>(c.images[layer]) + (size_t)y*c.pitch;
			// (the ladder is written out: through a run-time helper it is lowered as a switch, two more scalar branches for RGBA8)
			if (c.pixel_type == CFHIP_PIXEL_RGBA8)
				a = cf_load_channel<CFHIP_PIXEL_RGBA8>(row, x, 3u, of_u8);
			else if (c.pixel_type == CFHIP_PIXEL_RGBA32F)
				a = cf_load_channel<CFHIP_PIXEL_RGBA32F>(row, x, 3u, of_u8);
			else
				a = cf_load_channel<CFHIP_PIXEL_RGBA16F>(row, x, 3u, of_u8);
		}
		const bool seed = a > t;                       // false for a NaN
		if (active)
			seeds[(size_t)layer*c.width*c.height + (size_t)y*c.width + x] = seed ? (x | y << 16) : CFAB_NONE;
		n += (uint32_t)__popcll(__ballot(seed));
	}
	if (!results)
		return;
	if (threadIdx.x == 0 && n)
		atomicAdd(&sum, n);
	__syncthreads();
	if (threadIdx.x + threadIdx.y == 0 && sum)
		atomicAdd(&results[layer].seeds, sum);
}

template <bool WRAP>
__global__ void __launch_bounds__(WG)
cfhip_alpha_bleed_step_kernel(cfab_call c, uint32_t kx, uint32_t ky, const uint32_t* __restrict__ in, uint32_t* __restrict__ out)
{
	const uint32_t x = blockIdx.x*CFAB_WG_X + threadIdx.x, y = blockIdx.y*CFAB_WG_Y + threadIdx.y;
	if (x >= c.width || y >= c.height)
		return;
	const size_t base = (size_t)blockIdx.z*c.width*c.height;
	// (the largest key's low word is CFAB_NONE)
	out[base + (size_t)y*c.width + x] = (uint32_t)nearest<WRAP>(c, in + base, x, y, kx, ky);
}

template <class T>
__device__ __forceinline__ void copy_rgb(uint8_t* dst, const uint8_t* src)
{
	const T r = reinterpret_cast<const T*>(src)[0], g = reinterpret_cast<const T*>(src)[1], b = reinterpret_cast<const T*>(src)[2];
	reinterpret_cast<T*>(dst)[0] = r;
	reinterpret_cast<T*>(dst)[1] = g;
	reinterpret_cast<T*>(dst)[2] = b;
}

template <bool WRAP>
__global__ void __launch_bounds__(WG)
cfhip_alpha_bleed_fill_kernel(cfab_call c, uint32_t kx, uint32_t ky, uint32_t max_dist2, const uint32_t* __restrict__ in,
	cfhip_bleed_result* __restrict__ results)
{
	// the workgroup's sums: its four wavefronts meet here before one of them goes to memory
	__shared__ uint32_t sums[2];
	if (results && threadIdx.x + threadIdx.y == 0)
		sums[0] = sums[1] = 0;
	__syncthreads();
	const uint32_t gx = blockIdx.x*CFAB_WG_X + threadIdx.x, layer = blockIdx.z;
	const bool active = gx < c.width;
	const uint32_t x = active ? gx : 0u;               // every lane stays for the wave's sums
	uint32_t n = 0, far = 0;
	for (uint32_t j = 0; j < CFAB_ROWS; ++j) {
		const uint32_t y = (blockIdx.y*CFAB_ROWS + j)*CFAB_WG_Y + threadIdx.y;
		if (y >= c.height)
			break;                                     // the whole wavefront: it shares y
		const uint64_t best = nearest<WRAP>(c, in + (size_t)layer*c.width*c.height, x, y, kx, ky);
		const uint32_t s = (uint32_t)best, d2 = (uint32_t)(best >> 32);
		// a seed's own word has the key 0: a texel is a seed exactly when it found itself
		const bool fill = active && s != CFAB_NONE && s != (x | y << 16) && (max_dist2 == 0u || d2 <= max_dist2);
		if (fill) {
			uint8_t* base = static_cast<uint8_t*>(c.images[layer]);
			const size_t sx = s & 0xFFFFu, sy = s >> 16;
			if (c.pixel_type == CFHIP_PIXEL_RGBA8)
				copy_rgb<uint8_t>(base + (size_t)y*c.pitch + (size_t)x*4u, base + sy*c.pitch + sx*4u);
			else if (c.pixel_type == CFHIP_PIXEL_RGBA32F)
				copy_rgb<uint32_t>(base + (size_t)y*c.pitch + (size_t)x*16u, base + sy*c.pitch + sx*16u);
			else
				copy_rgb<unsigned short>(base + (size_t)y*c.pitch + (size_t)x*8u, base + sy*c.pitch + sx*8u);
			far = max(far, d2);
		}
		n += (uint32_t)__popcll(__ballot(fill));
	}
	if (!results)
		return;
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1)
		far = max(far, (uint32_t)__shfl_xor((int)far, m, 64));
	if (threadIdx.x == 0 && n) {
		atomicAdd(&sums[0], n);
		atomicMax(&sums[1], far);
	}
	__syncthreads();
	if (threadIdx.x + threadIdx.y == 0 && sums[0]) {
		atomicAdd(&results[layer].filled, sums[0]);
		atomicMax(&results[layer].max_dist2, sums[1]);
	}
}

// rows: of a wavefront (1 for a step; CFAB_ROWS for the two passes that count)
dim3 grid_of(const cfab_call& c, uint32_t layers, uint32_t rows)
{
	const uint32_t tall = CFAB_WG_Y*rows;
	return dim3((c.width + CFAB_WG_X - 1u)/CFAB_WG_X, (c.height + tall - 1u)/tall, layers);
}

} // namespace

extern "C" hipError_t cfhip_launch_alpha_bleed_seed(const cfab_call* call, uint32_t layers, float threshold, uint32_t* seeds,
	cfhip_bleed_result* results, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_alpha_bleed_seed_kernel, grid_of(*call, layers, CFAB_ROWS), dim3(CFAB_WG_X, CFAB_WG_Y), 0, stream, *call,
		threshold, seeds, results);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_alpha_bleed_step(const cfab_call* call, uint32_t layers, uint32_t step_x, uint32_t step_y,
	const uint32_t* seeds_in, uint32_t* seeds_out, hipStream_t stream)
{
	if (call->flags)
		hipLaunchKernelGGL(cfhip_alpha_bleed_step_kernel<true>, grid_of(*call, layers, 1u), dim3(CFAB_WG_X, CFAB_WG_Y), 0, stream,
			*call, step_x, step_y, seeds_in, seeds_out);
	else
		hipLaunchKernelGGL(cfhip_alpha_bleed_step_kernel<false>, grid_of(*call, layers, 1u), dim3(CFAB_WG_X, CFAB_WG_Y), 0, stream,
			*call, step_x, step_y, seeds_in, seeds_out);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_alpha_bleed_fill(const cfab_call* call, uint32_t layers, uint32_t step_x, uint32_t step_y,
	uint32_t max_dist2, const uint32_t* seeds_in, cfhip_bleed_result* results, hipStream_t stream)
{
	if (call->flags)
		hipLaunchKernelGGL(cfhip_alpha_bleed_fill_kernel<true>, grid_of(*call, layers, CFAB_ROWS), dim3(CFAB_WG_X, CFAB_WG_Y), 0,
			stream, *call, step_x, step_y, max_dist2, seeds_in, results);
	else
		hipLaunchKernelGGL(cfhip_alpha_bleed_fill_kernel<false>, grid_of(*call, layers, CFAB_ROWS), dim3(CFAB_WG_X, CFAB_WG_Y), 0,
			stream, *call, step_x, step_y, max_dist2, seeds_in, results);
	return hipGetLastError();
}
