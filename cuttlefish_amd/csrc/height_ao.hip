// height_ao.hip -- ambient occlusion from height maps: what a height field hides of the sky above
// each of its texels, from the horizon in D directions within R texels (include/cuttlefish_hip.h has the definition in
// full; tests/height_ao_ref.py restates it in numpy).
//
//   plane  the height channel of every texel, decoded to a float, not finite -> 0, into a plane of the context's scratch:
//          lossless (every decode is a float), it makes a call in place safe -- every height is read before the scan
//          writes anything -- and gives the scan one-word coalesced reads.  It also opens the records.
//   scan   a workgroup owns a tile of 64 x 16 texels (256 threads, R <= 16) or 64 x 64 (1024 threads, above) and stages
//          it and a halo of R texels in LDS once, a wrapped axis modulo its side, a texel outside an unwrapped surface as
//          a NaN.  A wavefront lies along x and owns four rows of the tile, so a sample step reads 64 consecutive words
//          of one LDS row: no bank conflict whatever the pitch.
//          The direction and the gain g(d, k) are uniform: they come from the call's table through scalar loads.  Per
//          sample and texel: one LDS read, a convert, an fma (height * h(q) - H(p): the product is exact, so this is
//          the subtraction), a multiply and an fmax in double; fmax drops the NaN of a sample that does not exist.
//          Records: a ballot and a shuffle minimum per wavefront, LDS atomics, one vector atomic add and one atomic
//          min per workgroup.
// All layers of a call share both launches (grid z).  No kernel here may use scratch, spill a vector register or use
// AGPRs (cuttlefish_amd/build.py).
#include "cf_texel.h"
#include "height_ao.h"

namespace {

constexpr uint32_t ONE_BITS = 0x3F800000u;         // 1.0f: v never exceeds it, and floats >= 0 order as their bits
constexpr uint32_t PLANE_ROWS = CFHAO_WG/CFHAO_TILE_W;
constexpr uint32_t OWN = CFHAO_OWN_ROWS;           // rows of a tile a wavefront owns: wave, wave + WAVES, ...

__global__ void __launch_bounds__(CFHAO_WG)
cfhip_height_ao_plane_kernel(cfhao_call c, float* __restrict__ plane, cfhip_height_ao_result* __restrict__ results)
{
	__shared__ float of_u8[256];
	const uint32_t v = threadIdx.y*CFHAO_TILE_W + threadIdx.x, layer = blockIdx.z;
	cf_fill_of_u8(of_u8, v, c.src_type == CFHIP_PIXEL_RGBA8);
	__syncthreads();
	if (results && v == 0 && blockIdx.x + blockIdx.y == 0) {
		cfhip_height_ao_result open;
		open.occluded = 0;
		open.darkest = ONE_BITS;
		open.reserved[0] = open.reserved[1] = 0;
		results[layer] = open;
	}
	const uint32_t x = blockIdx.x*CFHAO_TILE_W + threadIdx.x, y = blockIdx.y*PLANE_ROWS + threadIdx.y;
	if (x >= c.width || y >= c.height)
		return;
	const uint8_t* row = static_cast<const uint8_t*>(c.src[layer]) + (size_t)y*c.src_pitch;
	// (the ladder is written out: through a run-time helper it is lowered as a switch, two more scalar branches for RGBA8)
	float a;
	if (c.src_type == CFHIP_PIXEL_RGBA8)
		a = cf_load_channel<CFHIP_PIXEL_RGBA8>(row, x, c.channel, of_u8);
	else if (c.src_type == CFHIP_PIXEL_RGBA32F)
		a = cf_load_channel<CFHIP_PIXEL_RGBA32F>(row, x, c.channel, of_u8);
	else
		a = cf_load_channel<CFHIP_PIXEL_RGBA16F>(row, x, c.channel, of_u8);
	if (!__builtin_isfinite(a))
		a = 0.0f;
	plane[((size_t)layer*c.height + y)*c.width + x] = a;
}

// HALO: the largest radius of the build; WAVES: the wavefronts of its workgroup, four rows of the tile each.  Together
// they set the LDS (cfhao_lds_bytes) and so the workgroups that share a CU.
template <uint32_t HALO, uint32_t WAVES>
__global__ void __launch_bounds__(64u*WAVES)
cfhip_height_ao_scan_kernel(cfhao_call c, const float* __restrict__ plane, cfhip_height_ao_result* __restrict__ results)
{
	constexpr uint32_t P = CFHAO_TILE_W + 2u*HALO;     // words of an LDS row
	constexpr uint32_t TILE_H = OWN*WAVES;
	__shared__ float tile[P*(TILE_H + 2u*HALO)];
	__shared__ uint32_t record[2];                     // the workgroup's occluded texels and its darkest value
	static_assert(TILE_H == cfhao_tile_rows(HALO), "the tile that height_ao.h states");
	static_assert(sizeof(tile) + sizeof(record) == cfhao_lds_bytes(HALO), "the LDS that height_ao.h states");
	const uint32_t lane = threadIdx.x, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
	if (threadIdx.x + threadIdx.y == 0) {
		record[0] = 0;
		record[1] = ONE_BITS;
	}
	const uint32_t w = c.width, h = c.height, R = c.radius, layer = blockIdx.z;
	const uint32_t x0 = blockIdx.x*CFHAO_TILE_W, y0 = blockIdx.y*TILE_H;
	const uint32_t count = min(TILE_H, h - y0);        // rows of this tile
	const bool wrap_x = c.flags & CFHIP_HAO_WRAP_X, wrap_y = c.flags & CFHIP_HAO_WRAP_Y;
	const float* __restrict__ base = plane + (size_t)layer*w*h;
	// LDS texel (i, j) is the surface's (x0 - R + i, y0 - R + j): CFHAO_TILE_W + 2R columns of count + 2R rows
	for (uint32_t j = wave; j < count + 2u*R; j += WAVES) {
		int32_t yy = (int32_t)(y0 + j) - (int32_t)R;
		const bool row = cf_wrap_coord(yy, h, wrap_y);
		for (uint32_t i = lane; i < CFHAO_TILE_W + 2u*R; i += 64u) {
			int32_t xx = (int32_t)(x0 + i) - (int32_t)R;
			const bool there = cf_wrap_coord(xx, w, wrap_x) && row;
			tile[j*P + i] = there ? base[(size_t)yy*w + (size_t)xx] : __builtin_nanf("");
		}
	}
	__syncthreads();
	// A row past the tile's count reads LDS that nobody staged -- inside the array -- and its values are never stored
	const double hs = (double)c.height_scale, bias = (double)c.bias;
	const float* at = tile + (wave + R)*P + R + lane;
	double negHp[OWN], S[OWN];
	bool occluded[OWN];
#pragma unroll
	for (uint32_t r = 0; r < OWN; ++r) {
		negHp[r] = -(hs*(double)at[r*WAVES*P]);
		S[r] = 0.0;
		occluded[r] = false;
	}
	const cfhao_table* __restrict__ table = c.table;
	for (uint32_t d = 0; d < c.directions; ++d) {
		const int32_t step = table->dir[d].vy*(int32_t)P + table->dir[d].vx;
		const uint32_t reach = table->dir[d].reach;
		const double* __restrict__ gain = table->gain + table->dir[d].first;
		const double weight = table->dir[d].weight;
		double m[OWN];
#pragma unroll
		for (uint32_t r = 0; r < OWN; ++r)
			m[r] = -__builtin_inf();
		const float* q = at;
		for (uint32_t k = 0; k < reach; ++k) {
			q += step;
			const double g = gain[k];
#pragma unroll
			for (uint32_t r = 0; r < OWN; ++r)
				m[r] = fmax(m[r], fma(hs, (double)q[r*WAVES*P], negHp[r])*g);
		}
#pragma unroll
		for (uint32_t r = 0; r < OWN; ++r) {
			const double t = fmax(0.0, m[r] - bias);
			occluded[r] = occluded[r] || t > 0.0;
			const double vis = (c.flags & CFHIP_HAO_UNIFORM) ? 1.0 - t/sqrt(1.0 + t*t) : 1.0/(1.0 + t*t);
			S[r] = S[r] + weight*vis;
		}
	}
	const double strength = (double)c.strength;
	const uint32_t x = x0 + lane;
	uint32_t n = 0, dark = ONE_BITS;
#pragma unroll
	for (uint32_t r = 0; r < OWN; ++r) {
		const uint32_t j = wave + r*WAVES;
		const bool active = x < w && j < count;
		const double v = fmin(1.0, fmax(0.0, 1.0 - strength*(1.0 - S[r])));
		if (active) {
			cf_store_unit(static_cast<uint8_t*>(c.dst[layer]) + (size_t)(y0 + j)*c.dst_pitch, x, c.dst_type, c.channel_mask, v);
			dark = min(dark, __float_as_uint((float)v));
		}
		n += (uint32_t)__popcll(__ballot(active && occluded[r]));
	}
	if (!results)
		return;
#pragma unroll
	for (int s = 32; s > 0; s >>= 1)
		dark = min(dark, (uint32_t)__shfl_xor((int)dark, s));
	if (lane == 0) {
		if (n)
			atomicAdd(&record[0], n);
		if (dark < ONE_BITS)
			atomicMin(&record[1], dark);
	}
	__syncthreads();
	if (threadIdx.x + threadIdx.y == 0) {
		if (record[0])
			atomicAdd(&results[layer].occluded, record[0]);
		if (record[1] < ONE_BITS)
			atomicMin(&results[layer].darkest, record[1]);
	}
}

} // namespace

extern "C" hipError_t cfhip_launch_height_ao_plane(const cfhao_call* call, uint32_t layers, float* plane,
	cfhip_height_ao_result* results, hipStream_t stream)
{
	const dim3 grid((call->width + CFHAO_TILE_W - 1u)/CFHAO_TILE_W, (call->height + PLANE_ROWS - 1u)/PLANE_ROWS, layers);
	hipLaunchKernelGGL(cfhip_height_ao_plane_kernel, grid, dim3(CFHAO_TILE_W, PLANE_ROWS), 0, stream, *call, plane, results);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_height_ao_scan(const cfhao_call* call, uint32_t layers, const float* plane,
	cfhip_height_ao_result* results, hipStream_t stream)
{
	const uint32_t halo = call->radius <= CFHAO_HALO_CLASSES[0] ? CFHAO_HALO_CLASSES[0]
		: call->radius <= CFHAO_HALO_CLASSES[1] ? CFHAO_HALO_CLASSES[1] : CFHAO_HALO_CLASSES[2];
	const uint32_t rows = cfhao_tile_rows(halo);
	const dim3 grid((call->width + CFHAO_TILE_W - 1u)/CFHAO_TILE_W, (call->height + rows - 1u)/rows, layers);
	const dim3 block(CFHAO_TILE_W, rows/OWN);
	if (halo == CFHAO_HALO_CLASSES[0])
		hipLaunchKernelGGL((cfhip_height_ao_scan_kernel<CFHAO_HALO_CLASSES[0], CFHAO_TILE_H/OWN>), grid, block, 0, stream, *call,
			plane, results);
	else if (halo == CFHAO_HALO_CLASSES[1])
		hipLaunchKernelGGL((cfhip_height_ao_scan_kernel<CFHAO_HALO_CLASSES[1], CFHAO_TILE_H_WIDE/OWN>), grid, block, 0, stream,
			*call, plane, results);
	else
		hipLaunchKernelGGL((cfhip_height_ao_scan_kernel<CFHAO_HALO_CLASSES[2], CFHAO_TILE_H_WIDE/OWN>), grid, block, 0, stream,
			*call, plane, results);
	return hipGetLastError();
}
