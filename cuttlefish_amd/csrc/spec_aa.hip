// spec_aa.hip -- specular anti-aliasing: one channel of the levels of a roughness chain takes
// up the variance of the level-0 normals under each texel.  spec_aa.h states the definition and the tiling.
//
// A launch finishes five levels.  A workgroup owns one texel of the fifth: a 32 x 32 tile of its input grid (the last
// tile of a row or column runs to the edge, so the extended footprints of an odd end stay inside the tile).
//   first level   one thread per texel: it reads its 2 x 2 children (up to 3 x 3 at an odd end) straight from memory --
//                 level-0 texels, decoded, normalised and quantised in registers, or the moments the launch before left
//                 -- sums them in int64, stores the roughness, and leaves the sums in LDS
//   four more     out of LDS: first their sums, level by level (integer adds between barriers), then the roughness of
//                 all their texels in one trip -- finishing a level before summing the next would put four chains of
//                 double divisions and roots end to end while most of the workgroup waits
//   hand-over     the tile's last sums (32 bytes) go to the scratch: the next launch's input
// Level 0 is never staged: every texel is read once, by the one thread that needs it.  The records are summed in LDS and
// reach memory by one atomic add and one atomic max per workgroup.  Pixel types are template parameters, the storage
// of the normals picks one of four bodies at the kernel's entry, and PERCEPTUAL is read once per thread, outside every
// loop.  No kernel here may use scratch, spill a vector register or use AGPRs (cuttlefish_amd/build.py).
#include "cf_texel.h"
#include "spec_aa.h"

namespace {

constexpr int SRC_MOMENTS = -1;                    // NPIX of a stage that reads the scratch
constexpr int ROUGH_CONST = -1;                    // RPIX without a roughness map

__host__ __device__ __forceinline__ uint32_t level_dim(uint32_t d, uint32_t k)
{
	const uint32_t v = d >> k;
	return v ? v : 1u;
}

struct sums {
	long long x, y, z, a;
};

__device__ __forceinline__ void add(sums& s, const sums& t)
{
	s.x += t.x; s.y += t.y; s.z += t.z; s.a += t.a;
}

// the first three components as the definition decodes them (cf_texel.h), straight-line code
template <int PIX>
__device__ __forceinline__ void load_normal(const uint8_t* row, uint32_t x, const float* of_u8, double (&n)[3])
{
	const float4 v = cf_load_texel<PIX>(row, x, of_u8);
	n[0] = (double)v.x;
	n[1] = (double)v.y;
	n[2] = (double)v.z;
}

__device__ __forceinline__ long long quantise_rough(double r, bool perceptual)
{
	if (!(r >= 0.0))
		r = 0.0;
	if (r > 1.0)
		r = 1.0;
	const double alpha = perceptual ? r*r : r;
	// 0 ... 2^32: all but the last fit 32 bits, and a 32-bit conversion is one instruction
	const double q = rint(alpha*alpha*4294967296.0);
	return q >= 4294967296.0 ? 1ll << 32 : (long long)(unsigned int)q;
}

// No branch: the four texels of a thread are four independent chains of dependent double operations, and only
// straight-line code lets the scheduler interleave them.  A degenerate normal divides all the same; the quotients
// (NaN, inf) are dropped by the selects.
template <bool SIGN, bool RECZ>
__device__ __forceinline__ void quantise_normal(double (&n)[3], sums& q)
{
	double x = n[0], y = n[1], z = n[2];
	if (!SIGN) {
		x = x*2.0 - 1.0;
		y = y*2.0 - 1.0;
		z = z*2.0 - 1.0;
	}
	if (RECZ)
		z = sqrt(fmax(0.0, 1.0 - (x*x + y*y)));
	const double len = sqrt((x*x + y*y) + z*z);
	const bool ok = isfinite(len) && len > 0.0;
	const double qx = x/len, qy = y/len, qz = z/len;
	x = ok ? qx : 0.0;
	y = ok ? qy : 0.0;
	z = ok ? qz : 1.0;
	// |n| <= 1: the Q30 values fit 32 bits, and a 32-bit conversion is one instruction
	q.x = (int)rint(x*1073741824.0);
	q.y = (int)rint(y*1073741824.0);
	q.z = (int)rint(z*1073741824.0);
}

// the children of one texel of a stage's first level, summed
template <int NPIX, int RPIX, bool SIGN, bool RECZ>
struct source {
	const uint8_t* normals;            // the layer's level 0, or its moments
	const uint8_t* rough;
	unsigned long long normal_pitch, rough_pitch;
	const float* of_u8;
	long long qa_const;
	uint32_t channel, in_width;
	bool perceptual;

	__device__ __forceinline__ sums texel(uint32_t x, uint32_t y) const
	{
		sums q;
		if (NPIX == SRC_MOMENTS) {
			const cfsa_moments m = reinterpret_cast<const cfsa_moments*>(normals)[(size_t)y*in_width + x];
			q.x = m.sx; q.y = m.sy; q.z = m.sz; q.a = m.sa;
		} else {
			double n[3];
			load_normal<NPIX>(normals + (size_t)y*normal_pitch, x, of_u8, n);
			q.a = qa_const;
			if (RPIX != ROUGH_CONST)
				q.a = quantise_rough((double)cf_load_channel<RPIX>(rough + (size_t)y*rough_pitch, x, channel, of_u8), perceptual);
			quantise_normal<SIGN, RECZ>(n, q);
		}
		return q;
	}

	// columns [x0, x0 + nc), rows [y0, y0 + nr), nc and nr 1 to 3: the 2 x 2 of the interior without a branch (a
	// missing second column or row reads the first again and is not added), the third of an odd end after it
	__device__ __forceinline__ sums gather(uint32_t x0, uint32_t y0, uint32_t nc, uint32_t nr) const
	{
		const uint32_t x1 = x0 + (nc > 1u ? 1u : 0u), y1 = y0 + (nr > 1u ? 1u : 0u);
		sums s = texel(x0, y0);
		const sums b = texel(x1, y0), c = texel(x0, y1), d = texel(x1, y1);
		const sums zero = {0, 0, 0, 0};
		add(s, nc > 1u ? b : zero);
		add(s, nr > 1u ? c : zero);
		add(s, nc > 1u && nr > 1u ? d : zero);
		if (nc > 2u)
			for (uint32_t dy = 0; dy < nr; ++dy)
				add(s, texel(x0 + 2u, y0 + dy));
		if (nr > 2u)
			for (uint32_t dx = 0; dx < (nc > 2u ? 2u : nc); ++dx)
				add(s, texel(x0 + dx, y0 + 2u));
		return s;
	}
};

struct finisher {
	double scale, max_variance;
	bool perceptual;
	uint32_t clamped, saturated, max_added;            // of this thread, of one level

	// the stored roughness of a level's texel from its moments and its count of level-0 texels
	__device__ __forceinline__ float operator()(const sums& s, uint32_t n)
	{
		const double dn = (double)n, d30 = dn*1073741824.0, d32 = dn*4294967296.0;
		const double mx = (double)s.x/d30, my = (double)s.y/d30, mz = (double)s.z/d30;
		const double A2 = (double)s.a/d32;
		const double L2 = (mx*mx + my*my) + mz*mz;
		double v = 0.0;
		if (L2 < 1.0) {
			v = max_variance;
			bool hit = true;
			if (L2 > 0.0) {
				const double L = sqrt(L2), t = (1.0 - L2)/(L*(3.0 - L2));
				if (t < max_variance) {
					v = t;
					hit = false;
				}
			}
			clamped += hit ? 1u : 0u;
		}
		const double added = scale*v, sum = A2 + added;
		double a2 = sum;
		if (!(sum < 1.0)) {
			a2 = 1.0;
			++saturated;
		}
		const uint32_t bits = __float_as_uint((float)added);
		max_added = bits > max_added ? bits : max_added;
		double r = sqrt(a2);
		if (perceptual)
			r = sqrt(r);
		return (float)r;
	}

	// the thread's share of a level's record into the workgroup's, and a fresh start
	__device__ __forceinline__ void flush(uint32_t* rec)
	{
		if (clamped)
			atomicAdd(rec, clamped);
		if (saturated)
			atomicAdd(rec + 1, saturated);
		if (max_added)
			atomicMax(rec + 2, max_added);
		clamped = saturated = max_added = 0;
	}
};

// the level-0 texels under one axis of texel x of level k
__device__ __forceinline__ uint32_t span(uint32_t x, uint32_t k, uint32_t level_size, uint32_t size0)
{
	return x == level_size - 1u ? size0 - (x << k) : 1u << k;
}

template <int NPIX, int RPIX, bool SIGN, bool RECZ>
__device__ __forceinline__ void stage_body(const cfsa_call& c, uint32_t stage, const cfsa_moments* in, cfsa_moments* out,
	cfhip_spec_aa_result* results, long long (*lds)[CFSA_LDS_ENTRIES], uint32_t* rec, const float* of_u8)
{
	const uint32_t tid = threadIdx.x, layer = blockIdx.y;
	const uint32_t b = stage*CFSA_STAGE_LEVELS, last = c.levels_count - 1u;
	const uint32_t nl = last - b < CFSA_STAGE_LEVELS ? last - b : CFSA_STAGE_LEVELS;
	const uint32_t wb = level_dim(c.width, b), hb = level_dim(c.height, b);
	const uint32_t ntx = level_dim(c.width, b + CFSA_STAGE_LEVELS), nty = level_dim(c.height, b + CFSA_STAGE_LEVELS);
	const uint32_t tx = blockIdx.x % ntx, ty = blockIdx.x/ntx;
	const bool last_x = tx == ntx - 1u, last_y = ty == nty - 1u;
	if (tid < 16u)
		rec[tid] = 0;
	__syncthreads();

	source<NPIX, RPIX, SIGN, RECZ> src;
	src.channel = c.channel;
	src.in_width = wb;
	src.perceptual = c.flags & CFHIP_SPEC_AA_PERCEPTUAL;
	src.of_u8 = of_u8;
	src.normal_pitch = c.normal_pitch;
	src.rough_pitch = c.rough_pitch;
	src.rough = nullptr;
	src.qa_const = 0;
	if (NPIX == SRC_MOMENTS)
		src.normals = reinterpret_cast<const uint8_t*>(in + (size_t)layer*wb*hb);
	else {
		src.normals = static_cast<const uint8_t*>(c.normals[layer]);
		if (RPIX == ROUGH_CONST)
			src.qa_const = quantise_rough((double)c.base_roughness, src.perceptual);
		else
			src.rough = static_cast<const uint8_t*>(c.rough0[layer]);
	}
	finisher fin;
	fin.scale = (double)c.variance_scale;
	fin.max_variance = (double)c.max_variance;
	fin.perceptual = src.perceptual;
	fin.clamped = fin.saturated = fin.max_added = 0;

	// level j of the tile: its origin and its extent (its sums follow those of level j - 1 in LDS)
	struct tile_level {
		uint32_t k, wk, hk, ox, oy, nx, ny;
	};
	const auto level_of = [&](uint32_t j) {
		tile_level t;
		t.k = b + j;
		t.wk = level_dim(c.width, t.k);
		t.hk = level_dim(c.height, t.k);
		const uint32_t side = CFSA_TILE >> j;
		t.ox = tx*side;
		t.oy = ty*side;
		t.nx = (last_x ? t.wk : t.ox + side) - t.ox;
		t.ny = (last_y ? t.hk : t.oy + side) - t.oy;
		return t;
	};
	const auto finish_texel = [&](const tile_level& t, uint32_t lx, uint32_t ly, const sums& s) {
		const uint32_t X = t.ox + lx, Y = t.oy + ly;
		const uint32_t n = span(X, t.k, t.wk, c.width)*span(Y, t.k, t.hk, c.height);
		float* level = static_cast<float*>(c.levels[(size_t)layer*last + (t.k - 1u)]) + c.channel;
		level[((size_t)Y*t.wk + X)*4u] = fin(s, n);
	};

	// the first level: the children from memory, finished by the thread that summed them -- every thread has one
	const tile_level t1 = level_of(1u);
	for (uint32_t i = tid; i < t1.nx*t1.ny; i += CFSA_WG) {
		const uint32_t ly = i/t1.nx, lx = i - ly*t1.nx;
		const uint32_t X = t1.ox + lx, Y = t1.oy + ly;
		// the children: [2X, 2X + 2), the level's last texel up to the end of the level below
		const uint32_t nc = (X == t1.wk - 1u ? wb : 2u*X + 2u) - 2u*X, nr = (Y == t1.hk - 1u ? hb : 2u*Y + 2u) - 2u*Y;
		const sums s = src.gather(2u*X, 2u*Y, nc, nr);
		lds[0][i] = s.x; lds[1][i] = s.y; lds[2][i] = s.z; lds[3][i] = s.a;
		finish_texel(t1, lx, ly, s);
	}
	fin.flush(rec);
	__syncthreads();

	// the sums of the other levels, integers only: a level waits for the one below it, but for nobody's arithmetic
	uint32_t off = t1.nx*t1.ny, prev_off = 0;
	tile_level prev = t1;
#pragma unroll 1
	for (uint32_t j = 2; j <= nl; ++j) {
		const tile_level t = level_of(j);
		for (uint32_t i = tid; i < t.nx*t.ny; i += CFSA_WG) {
			const uint32_t ly = i/t.nx, lx = i - ly*t.nx;
			const uint32_t nc = (t.ox + lx == t.wk - 1u ? prev.nx : 2u*lx + 2u) - 2u*lx;
			const uint32_t nr = (t.oy + ly == t.hk - 1u ? prev.ny : 2u*ly + 2u) - 2u*ly;
			sums s = {0, 0, 0, 0};
			for (uint32_t dy = 0; dy < nr; ++dy)
				for (uint32_t dx = 0; dx < nc; ++dx) {
					const uint32_t e = prev_off + (2u*ly + dy)*prev.nx + 2u*lx + dx;
					s.x += lds[0][e]; s.y += lds[1][e]; s.z += lds[2][e]; s.a += lds[3][e];
				}
			const uint32_t e = off + i;
			lds[0][e] = s.x; lds[1][e] = s.y; lds[2][e] = s.z; lds[3][e] = s.a;
			if (j == CFSA_STAGE_LEVELS && out) {
				cfsa_moments m;
				m.sx = s.x; m.sy = s.y; m.sz = s.z; m.sa = s.a;
				out[(size_t)layer*ntx*nty + (size_t)ty*ntx + tx] = m;
			}
		}
		prev_off = off;
		prev = t;
		off += t.nx*t.ny;
		__syncthreads();
	}

	// ... and all their texels finished side by side: 85 of an inner tile, one trip
	for (uint32_t i = tid + t1.nx*t1.ny; i < off; i += CFSA_WG) {
		uint32_t j = 2u, r = i - t1.nx*t1.ny;
		tile_level t = level_of(j);
		while (r >= t.nx*t.ny) {
			r -= t.nx*t.ny;
			t = level_of(++j);
		}
		sums s;
		s.x = lds[0][i]; s.y = lds[1][i]; s.z = lds[2][i]; s.a = lds[3][i];
		const uint32_t ly = r/t.nx, lx = r - ly*t.nx;
		finish_texel(t, lx, ly, s);
		fin.flush(rec + (j - 1u)*3u);
	}
	__syncthreads();
	// rec[3 (j - 1) + f]: field f of level b + j
	if (results && tid < 3u*nl) {
		const uint32_t j = tid/3u, f = tid - j*3u, v = rec[tid];
		uint32_t* dst = reinterpret_cast<uint32_t*>(results + (size_t)layer*last + (b + j)) + f;
		if (v) {
			if (f == 2u)
				atomicMax(dst, v);
			else
				atomicAdd(dst, v);
		}
	}
}

template <int NPIX, int RPIX>
__global__ void __launch_bounds__(CFSA_WG)
cfhip_spec_aa_texel_kernel(cfsa_call c, cfsa_moments* __restrict__ out, cfhip_spec_aa_result* __restrict__ results)
{
	__shared__ long long lds[4][CFSA_LDS_ENTRIES];
	__shared__ uint32_t rec[16];
	__shared__ float of_u8[256];
	cf_fill_of_u8(of_u8, threadIdx.x, NPIX == CFHIP_PIXEL_RGBA8 || RPIX == CFHIP_PIXEL_RGBA8);
	// the storage of the normals is chosen here, once: each of the four bodies is straight-line code per texel
	const bool sign = c.flags & CFHIP_SPEC_AA_SIGNED_NORMALS, recz = c.flags & CFHIP_SPEC_AA_RECONSTRUCT_Z;
	if (!sign && !recz)
		stage_body<NPIX, RPIX, false, false>(c, 0u, nullptr, out, results, lds, rec, of_u8);
	else if (sign && !recz)
		stage_body<NPIX, RPIX, true, false>(c, 0u, nullptr, out, results, lds, rec, of_u8);
	else if (!sign)
		stage_body<NPIX, RPIX, false, true>(c, 0u, nullptr, out, results, lds, rec, of_u8);
	else
		stage_body<NPIX, RPIX, true, true>(c, 0u, nullptr, out, results, lds, rec, of_u8);
}

__global__ void __launch_bounds__(CFSA_WG)
cfhip_spec_aa_moment_kernel(cfsa_call c, uint32_t stage, const cfsa_moments* __restrict__ in, cfsa_moments* __restrict__ out,
	cfhip_spec_aa_result* __restrict__ results)
{
	__shared__ long long lds[4][CFSA_LDS_ENTRIES];
	__shared__ uint32_t rec[16];
	stage_body<SRC_MOMENTS, ROUGH_CONST, false, false>(c, stage, in, out, results, lds, rec, nullptr);
}

} // namespace

static_assert(sizeof(long long)*4u*CFSA_LDS_ENTRIES + 16u*4u == CFSA_LDS_BYTES, "the LDS DESIGN.md states");

extern "C" hipError_t cfhip_launch_spec_aa(const cfsa_call* call, uint32_t layers, uint32_t stage, const cfsa_moments* in,
	cfsa_moments* out, cfhip_spec_aa_result* results, hipStream_t stream)
{
	const uint32_t top = (stage + 1u)*CFSA_STAGE_LEVELS;
	const dim3 grid(level_dim(call->width, top)*level_dim(call->height, top), layers);
	if (stage)
		hipLaunchKernelGGL(cfhip_spec_aa_moment_kernel, grid, dim3(CFSA_WG), 0, stream, *call, stage, in, out, results);
	else
		cf_pixel_dispatch(call->normal_type, [&](auto npix) {
			constexpr int NPIX = decltype(npix)::value;
			if (!call->rough0)
				hipLaunchKernelGGL((cfhip_spec_aa_texel_kernel<NPIX, ROUGH_CONST>), grid, dim3(CFSA_WG), 0, stream, *call, out, results);
			else
				cf_pixel_dispatch(call->rough_type, [&](auto rpix) {
					hipLaunchKernelGGL((cfhip_spec_aa_texel_kernel<NPIX, decltype(rpix)::value>), grid, dim3(CFSA_WG), 0, stream, *call,
						out, results);
				});
		});
	return hipGetLastError();
}
