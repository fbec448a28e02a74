// alpha_sdf.hip -- a signed distance field from alpha: every source texel's Euclidean distance to
// the nearest texel of the other class (alpha > t or not), capped at K = spread + 1, signed, averaged over s x s tiles
// and stored with 0.5 at the silhouette (include/cuttlefish_hip.h has the definition in full; tests/alpha_sdf_ref.py
// restates it in numpy).  The cap makes the exact transform cheap and fully parallel:
//
//   classify  alpha read once per texel; the wavefront's ballot is one 64-bit word of the bit plane.  The inside count is
//             taken as alpha bleeding's seed pass counts: a wavefront walks CFSD_ROWS rows, the workgroup adds up in LDS,
//             one vector atomic per workgroup
//   row       per texel the distance to the nearest texel of the other class in its row, capped at K, from trailing and
//             leading zero counts on the row's words: its own and two on either side cover K <= 127.  One byte per
//             texel, the class in bit 7
//   column    a workgroup owns 64 columns x CFSD_TILE rows and stages their bytes and `spread` rows above and below in
//             LDS.  e = min over |dy| < K of dy^2 + g^2, g = 0 where that row's texel is of the other class, else its
//             byte (a byte of K adds nothing: dy^2 + K^2 > K^2).  dy walks outwards and the wavefront stops once
//             dy^2 >= e in every lane.  A byte read of 64 lanes is 16 dwords, four lanes each: no bank conflict.
//             At scale 1 the pass stores the field; else it writes e | class << 15
//   resolve   scale > 1: per output texel the sum of its s x s signed distances in double (exact), v and the store
// All layers of a call share every launch (grid z).  No kernel here may use scratch, spill a vector register or use
// AGPRs (cuttlefish_amd/build.py).
#include "cf_texel.h"
#include "alpha_sdf.h"

namespace {

constexpr uint32_t WG = CFSD_WG_X*CFSD_WG_Y;

// the signed distance of a texel: rho - 0.5 inside, 0.5 - rho outside, rho = (float)sqrt((double)e) -- the double
// square root is correctly rounded (mip_post.hip relies on the same)
__device__ __forceinline__ double signed_distance(uint32_t e, bool inside)
{
	const double rho = (double)(float)sqrt((double)e);
	return inside ? rho - 0.5 : 0.5 - rho;
}

// v of an output texel from the sum of its tile's signed distances, stored in the components of the mask
__device__ __forceinline__ void store_field(const cfsd_call& c, uint32_t layer, uint32_t x, uint32_t y, double sum)
{
	const double m = sum/(double)(c.scale*c.scale);
	double v = 0.5 + m/(2.0*(double)c.spread);
	v = v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
	cf_store_unit(static_cast<uint8_t*>(c.dst[layer]) + (size_t)y*c.dst_pitch, x, c.dst_type, c.channel_mask, v);
}

__global__ void __launch_bounds__(WG)
cfhip_alpha_sdf_classify_kernel(cfsd_call c, float t, uint64_t* __restrict__ plane, cfhip_sdf_result* __restrict__ results)
{
	__shared__ float of_u8[256];
	__shared__ uint32_t sum;                           // the workgroup's inside texels: its wavefronts meet here
	const uint32_t v = threadIdx.y*CFSD_WG_X + threadIdx.x;
	cf_fill_of_u8(of_u8, v, c.src_type == CFHIP_PIXEL_RGBA8);
	if (v == 0)
		sum = 0;
	__syncthreads();
	const uint32_t x = blockIdx.x*CFSD_WG_X + threadIdx.x, layer = blockIdx.z;
	const uint32_t words = (c.width + 63u) >> 6;
	const bool active = x < c.width;
	uint32_t n = 0;
	for (uint32_t j = 0; j < CFSD_ROWS; ++j) {
		const uint32_t y = (blockIdx.y*CFSD_ROWS + j)*CFSD_WG_Y + threadIdx.y;
		if (y >= c.height)
			break;                                     // the whole wavefront: it shares y
		float a = __builtin_nanf("");                  // a texel outside the surface is not inside
		if (active) {
			const uint8_t* row = static_cast<const uint8_t*>(c.src[layer]) + (size_t)y*c.src_pitch;
			// (the ladder is written out: through a run-time helper it is lowered as a switch, two more scalar branches for RGBA8)
			if (c.src_type == CFHIP_PIXEL_RGBA8)
				a = cf_load_channel<CFHIP_PIXEL_RGBA8>(row, x, 3u, of_u8);
			else if (c.src_type == CFHIP_PIXEL_RGBA32F)
				a = cf_load_channel<CFHIP_PIXEL_RGBA32F>(row, x, 3u, of_u8);
			else
				a = cf_load_channel<CFHIP_PIXEL_RGBA16F>(row, x, 3u, of_u8);
		}
		const uint64_t inside = __ballot(a > t);       // false for a NaN
		if (threadIdx.x == 0)
			plane[((size_t)layer*c.height + y)*words + blockIdx.x] = inside;
		n += (uint32_t)__popcll(inside);
	}
	if (!results)
		return;
	if (threadIdx.x == 0 && n)
		atomicAdd(&sum, n);
	__syncthreads();
	if (threadIdx.x + threadIdx.y == 0 && sum)
		atomicAdd(&results[layer].inside, sum);
}

// 64 texels of a row that repeats with period `width`, from position x0 (any sign) on: bit i = texel (x0 + i) mod width
__device__ __forceinline__ uint64_t periodic_bits(const uint64_t* __restrict__ row, uint32_t width, int32_t x0)
{
	int32_t p = cf_floor_mod(x0, width);
	uint64_t out = 0;
	for (uint32_t got = 0; got < 64u;) {
		const uint32_t s = (uint32_t)p & 63u;
		const uint32_t take = min(min(64u - s, width - (uint32_t)p), 64u - got);
		const uint64_t bits = row[(uint32_t)p >> 6] >> s;
		out |= (take == 64u ? bits : bits & ((1ull << take) - 1ull)) << got;
		got += take;
		p += (int32_t)take;
		if ((uint32_t)p == width)
			p = 0;
	}
	return out;
}

// WRAP: the x axis wraps.  Words and their masks are the same for the whole wavefront; each lane flips them by its own
// class, so that a set bit is a texel of the other class, and scans outwards.
template <bool WRAP>
__global__ void __launch_bounds__(WG)
cfhip_alpha_sdf_row_kernel(cfsd_call c, const uint64_t* __restrict__ plane, uint8_t* __restrict__ rows)
{
	const uint32_t y = blockIdx.y*CFSD_WG_Y + (uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
	if (y >= c.height)
		return;
	const uint32_t w = c.width, K = c.spread + 1u, words = (w + 63u) >> 6, word = blockIdx.x, lane = threadIdx.x;
	const size_t line = (size_t)blockIdx.z*c.height + y;
	const uint64_t* __restrict__ row = plane + line*words;
	uint64_t bits[5], valid[5];                        // the words at -2 ... +2 and the texels that exist in them
#pragma unroll
	for (int j = 0; j < 5; ++j) {
		if (WRAP) {
			bits[j] = periodic_bits(row, w, (int32_t)(word*64u) + (j - 2)*64);
			valid[j] = ~0ull;
		} else {
			const int32_t i = (int32_t)word + j - 2;
			const bool in = i >= 0 && i < (int32_t)words;
			const uint32_t texels = in ? w - (uint32_t)i*64u : 0u;
			bits[j] = in ? row[i] : 0ull;
			valid[j] = texels >= 64u ? ~0ull : (1ull << texels) - 1ull;
		}
	}
	const uint32_t inside = (uint32_t)(bits[2] >> lane) & 1u;
	const uint64_t flip = inside ? ~0ull : 0ull;
	uint64_t other[5];
#pragma unroll
	for (int j = 0; j < 5; ++j)
		other[j] = (bits[j] ^ flip) & valid[j];
	const uint64_t right = other[2] >> lane >> 1, left = other[2] << (63u - lane) << 1;
	const uint32_t dr = right ? (uint32_t)__builtin_ctzll(right) + 1u
		: other[3] ? 64u - lane + (uint32_t)__builtin_ctzll(other[3])
		: other[4] ? 128u - lane + (uint32_t)__builtin_ctzll(other[4]) : K;
	const uint32_t dl = left ? (uint32_t)__builtin_clzll(left) + 1u
		: other[1] ? lane + 1u + (uint32_t)__builtin_clzll(other[1])
		: other[0] ? lane + 65u + (uint32_t)__builtin_clzll(other[0]) : K;
	const uint32_t x = word*64u + lane;
	if (x < w)
		rows[line*w + x] = (uint8_t)(min(min(dl, dr), K) | inside << 7);
}

// FIELD: scale 1, the pass stores the field itself
template <bool FIELD>
__global__ void __launch_bounds__(WG)
cfhip_alpha_sdf_column_kernel(cfsd_call c, const uint8_t* __restrict__ rows, uint16_t* __restrict__ e16,
	cfhip_sdf_result* __restrict__ results)
{
	__shared__ uint8_t tile[CFSD_LDS_ROWS*64u];
	__shared__ uint32_t sum;                           // the workgroup's saturated texels
	if (threadIdx.x + threadIdx.y == 0)
		sum = 0;
	const uint32_t w = c.width, h = c.height, halo = c.spread, K2 = (c.spread + 1u)*(c.spread + 1u);
	const uint32_t y0 = blockIdx.y*CFSD_TILE, lane = threadIdx.x, x = blockIdx.x*64u + lane, layer = blockIdx.z;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
	const bool active = x < w, wrap = c.flags & CFHIP_SDF_WRAP_Y;
	const uint32_t count = min(CFSD_TILE, h - y0);     // rows of this tile
	const uint8_t* __restrict__ base = rows + (size_t)layer*w*h;
	// tile row i is surface row y0 - halo + i: modulo the height on a wrapped axis, not staged (and never read) outside
	for (uint32_t i = wave; i < count + 2u*halo; i += CFSD_WG_Y) {
		int32_t yy = (int32_t)(y0 + i) - (int32_t)halo;
		if (wrap)
			yy = cf_floor_mod(yy, h);
		else if (yy < 0 || yy >= (int32_t)h)
			continue;
		tile[i*64u + lane] = active ? base[(size_t)yy*w + x] : (uint8_t)0;
	}
	__syncthreads();
	uint32_t n = 0;
	for (uint32_t j = wave; j < count; j += CFSD_WG_Y) {
		const uint32_t y = y0 + j;
		const uint8_t* __restrict__ at = tile + (j + halo)*64u + lane;
		const uint32_t own = at[0], g = own & 127u;
		// (a lane past the width holds 0 and is done at once; a byte of K is K^2, the cap itself)
		uint32_t best = g*g;
		const uint32_t up = wrap ? halo : min(halo, y), down = wrap ? halo : min(halo, h - 1u - y);
		// two steps per trip, their four reads issued before the first is used.  A row that does not exist (or lies
		// past the halo) is replaced by the texel's own row: same class, so its candidate is s^2 + g^2 > g^2 >= best
		for (uint32_t d = 1; d <= halo; d += 2u) {
			if (!__any(d*d < best))
				break;
			uint32_t b[4];
#pragma unroll
			for (uint32_t k = 0; k < 2u; ++k) {
				const uint32_t s = d + k;
				b[2u*k] = at[s <= up ? -(int32_t)(s*64u) : 0];
				b[2u*k + 1u] = at[s <= down ? (int32_t)(s*64u) : 0];
			}
#pragma unroll
			for (uint32_t i = 0; i < 4u; ++i) {
				const uint32_t s = d + i/2u, t = ((b[i] ^ own) & 128u) ? 0u : b[i] & 127u;
				best = min(best, s*s + t*t);
			}
		}
		n += (uint32_t)__popcll(__ballot(active && best == K2));
		if (active) {
			if (FIELD)
				store_field(c, layer, x, y, signed_distance(best, own >> 7));
			else
				e16[((size_t)layer*h + y)*w + x] = (uint16_t)(best | (own & 128u) << 8);
		}
	}
	if (!results)
		return;
	if (lane == 0 && n)
		atomicAdd(&sum, n);
	__syncthreads();
	if (threadIdx.x + threadIdx.y == 0 && sum)
		atomicAdd(&results[layer].saturated, sum);
}

// one output texel per lane: its s rows of s values are s / 2 aligned dwords each (width is a multiple of s, s is even)
__global__ void __launch_bounds__(WG)
cfhip_alpha_sdf_resolve_kernel(cfsd_call c, const uint16_t* __restrict__ e16)
{
	const uint32_t s = c.scale, ow = c.width/s, oh = c.height/s;
	const uint32_t x = blockIdx.x*CFSD_WG_X + threadIdx.x, y = blockIdx.y*CFSD_WG_Y + threadIdx.y, layer = blockIdx.z;
	if (x >= ow || y >= oh)
		return;
	const uint16_t* __restrict__ from = e16 + ((size_t)layer*c.height + (size_t)y*s)*c.width + (size_t)x*s;
	double sum = 0.0;
	for (uint32_t r = 0; r < s; ++r) {
		const uint32_t* __restrict__ pairs = reinterpret_cast<const uint32_t*>(from + (size_t)r*c.width);
		for (uint32_t k = 0; k < s/2u; ++k) {
			const uint32_t p = pairs[k];
			sum += signed_distance(p & 0x7FFFu, p >> 15 & 1u);
			sum += signed_distance(p >> 16 & 0x7FFFu, p >> 31);
		}
	}
	store_field(c, layer, x, y, sum);
}

} // namespace

extern "C" hipError_t cfhip_launch_alpha_sdf_classify(const cfsd_call* call, uint32_t layers, float threshold, uint64_t* plane,
	cfhip_sdf_result* results, hipStream_t stream)
{
	const uint32_t tall = CFSD_WG_Y*CFSD_ROWS;
	hipLaunchKernelGGL(cfhip_alpha_sdf_classify_kernel, dim3((call->width + 63u)/64u, (call->height + tall - 1u)/tall, layers),
		dim3(CFSD_WG_X, CFSD_WG_Y), 0, stream, *call, threshold, plane, results);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_alpha_sdf_row(const cfsd_call* call, uint32_t layers, const uint64_t* plane, uint8_t* rows,
	hipStream_t stream)
{
	const dim3 grid((call->width + 63u)/64u, (call->height + CFSD_WG_Y - 1u)/CFSD_WG_Y, layers);
	if (call->flags & CFHIP_SDF_WRAP_X)
		hipLaunchKernelGGL(cfhip_alpha_sdf_row_kernel<true>, grid, dim3(CFSD_WG_X, CFSD_WG_Y), 0, stream, *call, plane, rows);
	else
		hipLaunchKernelGGL(cfhip_alpha_sdf_row_kernel<false>, grid, dim3(CFSD_WG_X, CFSD_WG_Y), 0, stream, *call, plane, rows);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_alpha_sdf_column(const cfsd_call* call, uint32_t layers, const uint8_t* rows, uint16_t* e,
	cfhip_sdf_result* results, hipStream_t stream)
{
	const dim3 grid((call->width + 63u)/64u, (call->height + CFSD_TILE - 1u)/CFSD_TILE, layers);
	if (call->scale == 1u)
		hipLaunchKernelGGL(cfhip_alpha_sdf_column_kernel<true>, grid, dim3(CFSD_WG_X, CFSD_WG_Y), 0, stream, *call, rows, e, results);
	else
		hipLaunchKernelGGL(cfhip_alpha_sdf_column_kernel<false>, grid, dim3(CFSD_WG_X, CFSD_WG_Y), 0, stream, *call, rows, e, results);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_alpha_sdf_resolve(const cfsd_call* call, uint32_t layers, const uint16_t* e, hipStream_t stream)
{
	const uint32_t ow = call->width/call->scale, oh = call->height/call->scale;
	hipLaunchKernelGGL(cfhip_alpha_sdf_resolve_kernel, dim3((ow + 63u)/64u, (oh + CFSD_WG_Y - 1u)/CFSD_WG_Y, layers),
		dim3(CFSD_WG_X, CFSD_WG_Y), 0, stream, *call, e);
	return hipGetLastError();
}
