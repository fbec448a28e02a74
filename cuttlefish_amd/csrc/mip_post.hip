// mip_post.hip -- the repairs of a generated mip chain before it is encoded: every level's
// alpha scaled so that its alpha-test coverage matches level 0's, and every normal renormalised.
//
// Coverage is an integer count of texels with fl32(alpha * s) >= t, and the scale of a level is defined as an extremum
// over float32 bit patterns (the smallest s above 1 whose count reaches the target, or the largest below 1 whose count
// does not pass it).  The count is monotone in s, so the extremum is found by narrowing a range of bit patterns: the
// 2^24 patterns between 1 and 4 (or 1/4 and 1) split 16 ways per pass, 6 passes.  All surfaces of a call share every
// launch; the workgroups are numbered across the surfaces and find theirs by binary search, as the batched encoders do.
//
//   gather  level 0 and every level: alpha read once; the levels' alpha into a compact float plane (4 of the 16 bytes
//           of a texel matter, and the six passes after this one read 4 B per texel for it); counts at s = 1, 1/4, 4
//   decide  one thread per level: target, direction, clamps; later the narrowed range, at the end rules 4 and 5
//   count   15 candidate scales per alpha read: one ballot and population count per candidate, wave-uniform sums, one
//           vector atomic add per wavefront (lane j adds candidate j's count: 64 contiguous bytes)
//   apply   alpha scale and renormalisation fused, in place
// No kernel here may use scratch, spill a vector register or use AGPRs (cuttlefish_amd/build.py).
#include "cf_texel.h"
#include "mip_post.h"

namespace {

__device__ __forceinline__ uint32_t resolve(const cfmp_surf* tab, uint32_t n, uint32_t wg)
{
	uint32_t lo = 0, hi = n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1u) >> 1;
		if (tab[mid].wg_begin <= wg) lo = mid; else hi = mid - 1u;
	}
	return lo;
}

// The alpha components of a thread's texels as stored, zero-extended.  All loads are issued before any value is
// converted, with no branch between them: a texel past the end reads the last one (it is not counted), and the pixel
// type and the row layout are chosen outside the loop.  (One load per counted texel serialises eight round trips to
// memory per wavefront.)  TIGHT: the rows follow each other without a gap, so the texel index is the position and no
// division by the width is needed.
template <int PIX, bool TIGHT>
__device__ __forceinline__ void load_alpha_raw(const cfmp_surf& s, uint32_t base, uint32_t (&raw)[CFMP_PER_THREAD])
{
#pragma unroll
	for (uint32_t i = 0; i < CFMP_PER_THREAD; ++i) {
		const uint32_t at = base + i*CFMP_WG, idx = at < s.n ? at : s.n - 1u;
		uint32_t x = idx, y = 0;
		if (!TIGHT) {
			y = idx/s.width;
			x = idx - y*s.width;
		}
		const uint8_t* row = s.pixels + (size_t)y*s.pitch;
		raw[i] = cf_channel_raw<PIX>(row, x, 3u);
	}
}

template <int PIX>
__device__ __forceinline__ void load_alpha_raw(const cfmp_surf& s, uint32_t base, uint32_t (&raw)[CFMP_PER_THREAD])
{
	if (s.pitch == (unsigned long long)s.width*cf_pixel_size(PIX))
		load_alpha_raw<PIX, true>(s, base, raw);
	else
		load_alpha_raw<PIX, false>(s, base, raw);
}

// lane j of the wavefront adds cnt[j]: one atomic instruction per wavefront
template <uint32_t N>
__device__ __forceinline__ void add_counts(const uint32_t (&cnt)[N], uint32_t used, uint32_t* dst)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t v = 0;
#pragma unroll
	for (uint32_t j = 0; j < N; ++j)
		v = lane == j ? cnt[j] : v;
	if (lane < used && v)
		atomicAdd(dst + lane, v);
}

__global__ void __launch_bounds__(CFMP_WG)
cfhip_mip_post_gather_kernel(const cfmp_surf* __restrict__ tab, uint32_t nsurf, uint32_t nlev, float t, float s0, float s1,
	float s2, uint32_t ncand, uint32_t cstride, float* __restrict__ plane, uint32_t* __restrict__ counters)
{
	__shared__ float of_u8[256];
	const uint32_t si = resolve(tab, nsurf, blockIdx.x);
	const cfmp_surf s = tab[si];
	if (s.pixel_type == CFHIP_PIXEL_RGBA8) {
		cf_fill_of_u8(of_u8, threadIdx.x, true);
		__syncthreads();
	}
	const uint32_t base = (blockIdx.x - s.wg_begin)*CFMP_CHUNK + threadIdx.x;
	const bool keep = plane && si < nlev;
	uint32_t raw[CFMP_PER_THREAD];
	// (not cf_pixel_dispatch: through a lambda the compiler merges the six bodies' loads into fewer, address-selected ones)
	if (s.pixel_type == CFHIP_PIXEL_RGBA8)
		load_alpha_raw<CFHIP_PIXEL_RGBA8>(s, base, raw);
	else if (s.pixel_type == CFHIP_PIXEL_RGBA32F)
		load_alpha_raw<CFHIP_PIXEL_RGBA32F>(s, base, raw);
	else
		load_alpha_raw<CFHIP_PIXEL_RGBA16F>(s, base, raw);
	uint32_t cnt[3] = {0, 0, 0};
#pragma unroll
	for (uint32_t i = 0; i < CFMP_PER_THREAD; ++i) {
		const uint32_t idx = base + i*CFMP_WG;
		float a = __builtin_nanf("");              // a texel past the end never counts
		if (idx < s.n) {
			a = cf_channel_of_raw(s.pixel_type, raw[i], of_u8);
			if (keep)
				plane[s.plane_off + idx] = a;
		}
		cnt[0] += (uint32_t)__popcll(__ballot(a*s0 >= t));
		cnt[1] += (uint32_t)__popcll(__ballot(a*s1 >= t));
		cnt[2] += (uint32_t)__popcll(__ballot(a*s2 >= t));
	}
	add_counts(cnt, ncand, counters + (size_t)si*cstride);
}

__global__ void __launch_bounds__(CFMP_WG)
cfhip_mip_post_count_kernel(const cfmp_surf* __restrict__ tab, uint32_t nlev, float t, const cfmp_state* __restrict__ state,
	const float* __restrict__ plane, uint32_t* __restrict__ counters)
{
	const uint32_t si = resolve(tab, nlev, blockIdx.x);
	const cfmp_state st = state[si];
	if (st.dir == 0)
		return;
	const cfmp_surf s = tab[si];
	const uint32_t base = (blockIdx.x - s.wg_begin)*CFMP_CHUNK + threadIdx.x;
	const float* a_of = plane + s.plane_off;
	const uint32_t step = (st.hi - st.lo) >> 4;
	float a[CFMP_PER_THREAD];
#pragma unroll
	for (uint32_t i = 0; i < CFMP_PER_THREAD; ++i) {
		const uint32_t idx = base + i*CFMP_WG;
		a[i] = idx < s.n ? a_of[idx] : __builtin_nanf("");
	}
	uint32_t cnt[CFMP_SLOTS];
	cnt[0] = 0;
#pragma unroll
	for (uint32_t j = 1; j < CFMP_SLOTS; ++j) {
		const float sc = __uint_as_float(st.lo + j*step);
		uint32_t c = 0;
#pragma unroll
		for (uint32_t i = 0; i < CFMP_PER_THREAD; ++i)
			c += (uint32_t)__popcll(__ballot(a[i]*sc >= t));
		cnt[j] = c;
	}
	add_counts(cnt, CFMP_SLOTS, counters + (size_t)si*CFMP_SLOTS);
}

__device__ __forceinline__ uint32_t dist(uint32_t a, uint32_t b)
{
	return a > b ? a - b : b - a;
}

// rules 4 and 5 of the scale, and the level's record
__device__ __forceinline__ void finish(cfmp_state& st, uint32_t bits, uint32_t count, cfhip_mip_post_result* res)
{
	if (count == st.c1) {                              // a scale that does not move the count is not applied
		bits = CFMP_BITS_ONE;
		count = st.c1;
	}
	st.dir = 0;
	st.scale_bits = bits;
	res->scale = __uint_as_float(bits);
	res->target = st.target;
	res->count_before = st.c1;
	res->count_after = count;
}

__global__ void __launch_bounds__(CFMP_WG)
cfhip_mip_post_decide_kernel(const cfmp_surf* __restrict__ tab, uint32_t nlev, int first, cfmp_state* __restrict__ state,
	uint32_t* __restrict__ counters, cfhip_mip_post_result* __restrict__ results)
{
	const uint32_t i = blockIdx.x*CFMP_WG + threadIdx.x;
	if (i >= nlev)
		return;
	uint32_t* c = counters + (size_t)i*CFMP_SLOTS;
	cfmp_state st = state[i];
	if (first) {
		const cfmp_surf s = tab[i];
		const unsigned long long c0 = counters[(size_t)s.ref*CFMP_SLOTS], n0 = tab[s.ref].n;
		const uint32_t c1 = c[0], cmin = c[1], cmax = c[2];
		st.target = (uint32_t)((c0*s.n + n0/2u)/n0);
		st.c1 = c1;
		st.lo = st.hi = st.cnt_lo = st.cnt_hi = 0;
		if (c1 == st.target)
			finish(st, CFMP_BITS_ONE, c1, results + i);
		else if (c1 < st.target) {
			if (cmax < st.target)
				finish(st, CFMP_BITS_MAX, cmax, results + i);
			else {
				st.lo = CFMP_BITS_ONE; st.cnt_lo = c1; st.hi = CFMP_BITS_MAX; st.cnt_hi = cmax; st.dir = 1;
			}
		} else {
			if (cmin > st.target)
				finish(st, CFMP_BITS_MIN, cmin, results + i);
			else {
				st.lo = CFMP_BITS_MIN; st.cnt_lo = cmin; st.hi = CFMP_BITS_ONE; st.cnt_hi = c1; st.dir = -1;
			}
		}
		c[0] = c[1] = c[2] = 0;
		state[i] = st;
		return;
	}
	if (st.dir == 0)
		return;
	// count(lo + j*step) for j = 0..16, non-decreasing; up: the first j at or above the target, down: the last j at
	// or below it.  Either way the answer's two candidates stay inside [lo + (j-1)*step, lo + j*step].
	const uint32_t step = (st.hi - st.lo) >> 4, T = st.target;
	uint32_t j = 1, below = st.cnt_lo, above = st.cnt_hi;
	if (st.dir > 0) {
		for (; j < CFMP_SLOTS && c[j] < T; ++j)
			below = c[j];
	} else {
		for (; j < CFMP_SLOTS && c[j] <= T; ++j)
			below = c[j];
	}
	if (j < CFMP_SLOTS)
		above = c[j];
	st.lo += (j - 1u)*step;
	st.hi = st.lo + step;
	st.cnt_lo = below;
	st.cnt_hi = above;
	for (uint32_t k = 1; k < CFMP_SLOTS; ++k)
		c[k] = 0;
	if (step == 1u) {
		// d = lo, u = hi: the nearer count wins, a tie goes to u
		if (dist(st.cnt_hi, T) <= dist(st.cnt_lo, T))
			finish(st, st.hi, st.cnt_hi, results + i);
		else
			finish(st, st.lo, st.cnt_lo, results + i);
	}
	state[i] = st;
}

template <bool NORM>
__global__ void __launch_bounds__(CFMP_WG)
cfhip_mip_post_apply_kernel(const cfmp_surf* __restrict__ tab, uint32_t nlev, uint32_t flags, const cfmp_state* __restrict__ state)
{
	const uint32_t si = resolve(tab, nlev, blockIdx.x);
	const float sc = state ? __uint_as_float(state[si].scale_bits) : 1.0f;
	const bool scale = sc != 1.0f;
	if (!NORM && !scale)
		return;                                        // the level keeps every byte
	const cfmp_surf s = tab[si];
	const uint32_t base = (blockIdx.x - s.wg_begin)*CFMP_CHUNK + threadIdx.x;
	const bool sign = flags & CFHIP_MIP_POST_SIGNED_NORMALS;
	float4* px = reinterpret_cast<float4*>(const_cast<uint8_t*>(s.pixels));
#pragma unroll
	for (uint32_t i = 0; i < CFMP_PER_THREAD; ++i) {
		const uint32_t idx = base + i*CFMP_WG;
		if (idx >= s.n)
			continue;
		if (!NORM) {
			float* ap = reinterpret_cast<float*>(px + idx) + 3;
			const float a = *ap*sc;
			*ap = a < 1.0f ? a : 1.0f;                 // fminf(a, 1): a NaN becomes 1
			continue;
		}
		float4 v = px[idx];
		if (scale) {
			const float a = v.w*sc;
			v.w = a < 1.0f ? a : 1.0f;
		}
		double x = (double)v.x, y = (double)v.y, z = (double)v.z;
		if (!sign) {
			x = x*2.0 - 1.0;
			y = y*2.0 - 1.0;
			z = z*2.0 - 1.0;
		}
		const double len = sqrt((x*x + y*y) + z*z);
		if (isfinite(len) && len > 0.0) {
			x = x/len;
			y = y/len;
			z = z/len;
		} else {
			x = y = 0.0;
			z = 1.0;
		}
		if (!sign) {
			x = x*0.5 + 0.5;
			y = y*0.5 + 0.5;
			z = z*0.5 + 0.5;
		}
		v.x = (float)x;
		v.y = (float)y;
		v.z = (float)z;
		px[idx] = v;
	}
}

} // namespace

extern "C" hipError_t cfhip_launch_mip_post_gather(const cfmp_surf* tab, uint32_t nsurf, uint32_t nlev, uint32_t total_wg,
	float threshold, float s0, float s1, float s2, uint32_t ncand, uint32_t cstride, float* plane, uint32_t* counters,
	hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_mip_post_gather_kernel, dim3(total_wg), dim3(CFMP_WG), 0, stream, tab, nsurf, nlev, threshold,
		s0, s1, s2, ncand, cstride, plane, counters);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_mip_post_count(const cfmp_surf* tab, uint32_t nlev, uint32_t total_wg, float threshold,
	const cfmp_state* state, const float* plane, uint32_t* counters, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_mip_post_count_kernel, dim3(total_wg), dim3(CFMP_WG), 0, stream, tab, nlev, threshold, state,
		plane, counters);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_mip_post_decide(const cfmp_surf* tab, uint32_t nlev, int first, cfmp_state* state,
	uint32_t* counters, cfhip_mip_post_result* results, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_mip_post_decide_kernel, dim3((nlev + CFMP_WG - 1u)/CFMP_WG), dim3(CFMP_WG), 0, stream, tab,
		nlev, first, state, counters, results);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_mip_post_apply(const cfmp_surf* tab, uint32_t nlev, uint32_t total_wg, uint32_t flags,
	const cfmp_state* state, hipStream_t stream)
{
	if (flags & CFHIP_MIP_POST_NORMALIZE)
		hipLaunchKernelGGL(cfhip_mip_post_apply_kernel<true>, dim3(total_wg), dim3(CFMP_WG), 0, stream, tab, nlev, flags, state);
	else
		hipLaunchKernelGGL(cfhip_mip_post_apply_kernel<false>, dim3(total_wg), dim3(CFMP_WG), 0, stream, tab, nlev, flags, state);
	return hipGetLastError();
}
