// envmap.hip -- environment maps for image-based lighting: an equirectangular panorama onto the
// six faces of a cube, the cube's GGX-prefiltered mip chain, and its projection on nine spherical-harmonic coefficients.
// envmap.h has the shared definitions (faces, directions, the seamless fetch, sum64); include/cuttlefish_hip.h has them in
// full and tests/envmap_ref.py restates them in numpy.  Every formula is IEEE double in the stated order, so the kernels
// return the twin's bits -- but for the panorama's atan2 and asin, which are the device library's.
//
//   equirect   one output texel per lane, the six faces in grid z: q x q sub-samples, each a direction, two angles and a
//              bilinear fetch from the panorama (x wrapped, y clamped)
//   prefilter  one wavefront per output texel, four per workgroup; lane j takes the records i = j mod 64 of the level's
//              sample table, staged in LDS CFENV_CHUNK at a time: the record's direction in the texel's frame, its face
//              and (s, t) once, then a seamless bilinear fetch from two source levels.  The lanes' sums meet in the xor
//              butterfly that sum64 names.  The chain's pointers sit in LDS beside the table.
//   copy       a roughness-0 level: the source level's bits
//   sh9 rows   one wavefront per face row: 37 sums per lane (9 basis values x RGBA, and the solid angle), the butterfly,
//              one record per row
//   sh9 final  the rows added in (face, y) order, one value per lane, and the normalisation
//   brdf lut   (section 4.27) one wavefront per texel of the split sum's second factor: the prefilter's frame around a
//              Hammersley table -- GGX scale and bias, and with sheen the Charlie albedo
//   irradiance (section 4.27) one output texel per lane: the diffuse term evaluated from the record sh9 final left
// No kernel here may use scratch, spill a vector register or use AGPRs (cuttlefish_amd/build.py).
#include "cf_texel.h"
#include "envmap.h"

namespace {

constexpr uint32_t WG = CFENV_WG_X*CFENV_WG_Y;

__device__ __forceinline__ void face_dir(uint32_t f, double s, double t, double& x, double& y, double& z)
{
	x = f == 0u ? 1.0 : f == 1u ? -1.0 : f == 5u ? -s : s;
	y = f == 2u ? 1.0 : f == 3u ? -1.0 : -t;
	z = f == 0u ? -s : f == 1u ? s : f == 2u ? t : f == 3u ? -t : f == 4u ? 1.0 : -1.0;
}

__device__ __forceinline__ void dir_to_face(double x, double y, double z, uint32_t& f, double& s, double& t)
{
	const double ax = fabs(x), ay = fabs(y), az = fabs(z);
	const bool isx = ax >= ay && ax >= az, isy = !isx && ay >= az;
	const bool neg = isx ? x < 0.0 : isy ? y < 0.0 : z < 0.0;
	f = (isx ? 0u : isy ? 2u : 4u) + (neg ? 1u : 0u);
	const double ma = isx ? ax : isy ? ay : az;
	const double a = isx ? (neg ? z : -z) : isy ? x : (neg ? -x : x);
	const double b = isy ? (neg ? -z : z) : -y;
	s = a/ma;
	t = b/ma;
}

// floor(p) held to [lo, hi]; a NaN becomes lo
__device__ __forceinline__ int32_t floor_index(double p, int32_t lo, int32_t hi, double* floored = nullptr)
{
	double q = floor(p);
	q = q >= (double)lo ? q : (double)lo;
	q = q > (double)hi ? (double)hi : q;
	if (floored)
		*floored = q;
	return (int32_t)q;
}

__device__ __forceinline__ double unit_coord(double at, double dn)
{
	return (2.0*at)/dn - 1.0;
}

// the texel that tap (i, j) of face f stands for, as an index into a face set of n x n faces, face after face
__device__ __forceinline__ void resolve_tap(uint32_t f, int32_t i, int32_t j, uint32_t n, double dn, uint32_t& face, uint32_t& at)
{
	if (i >= 0 && i < (int32_t)n && j >= 0 && j < (int32_t)n) {
		face = f;
		at = (uint32_t)j*n + (uint32_t)i;
		return;
	}
	double x, y, z, s, t;
	face_dir(f, unit_coord((double)i + 0.5, dn), unit_coord((double)j + 0.5, dn), x, y, z);
	dir_to_face(x, y, z, face, s, t);
	const int32_t i2 = floor_index(((s + 1.0)*0.5)*dn, 0, (int32_t)n - 1);
	const int32_t j2 = floor_index(((t + 1.0)*0.5)*dn, 0, (int32_t)n - 1);
	at = (uint32_t)j2*n + (uint32_t)i2;
}

// the seamless bilinear fetch of (f, s, t) from one level; faces: that level's six pointers, `stride` apart in the table
__device__ __forceinline__ void fetch(const float4* const* faces, uint32_t stride, uint32_t n, uint32_t f, double s, double t,
	double out[4])
{
	const double dn = (double)n;
	const double px = ((s + 1.0)*0.5)*dn - 0.5, py = ((t + 1.0)*0.5)*dn - 0.5;
	double x0f, y0f;
	const int32_t x0 = floor_index(px, -1, (int32_t)n - 1, &x0f), y0 = floor_index(py, -1, (int32_t)n - 1, &y0f);
	const double fx = px - x0f, fy = py - y0f;
	float4 c[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		uint32_t face, at;
		resolve_tap(f, x0 + (k & 1), y0 + (k >> 1), n, dn, face, at);
		c[k] = faces[face*stride][at];
	}
	const double gx = 1.0 - fx, gy = 1.0 - fy;
	out[0] = (((double)c[0].x*gx + (double)c[1].x*fx)*gy) + (((double)c[2].x*gx + (double)c[3].x*fx)*fy);
	out[1] = (((double)c[0].y*gx + (double)c[1].y*fx)*gy) + (((double)c[2].y*gx + (double)c[3].y*fx)*fy);
	out[2] = (((double)c[0].z*gx + (double)c[1].z*fx)*gy) + (((double)c[2].z*gx + (double)c[3].z*fx)*fy);
	out[3] = (((double)c[0].w*gx + (double)c[1].w*fx)*gy) + (((double)c[2].w*gx + (double)c[3].w*fx)*fy);
}

// sum64's second half: p_j += p_{j xor 32}, 16, 8, 4, 2, 1
__device__ __forceinline__ double butterfly(double p)
{
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1)
		p = p + __shfl_xor(p, m, 64);
	return p;
}

// ---- part 1 -------------------------------------------------------------------------------------------------------------
// component by component: the panorama is the caller's memory, at any alignment its components allow
__device__ __forceinline__ void panorama_texel(const uint8_t* row, uint32_t x, int32_t type, const float* of_u8, double out[4])
{
	cf_pixel_dispatch(type, [&](auto pix) {
		const float4 v = cf_load_texel<decltype(pix)::value, false>(row, x, of_u8);
		out[0] = (double)v.x; out[1] = (double)v.y; out[2] = (double)v.z; out[3] = (double)v.w;
	});
}

__global__ void __launch_bounds__(WG)
cfhip_equirect_to_cube_kernel(const uint8_t* __restrict__ src, int32_t type, uint32_t W, uint32_t H, unsigned long long pitch,
	void* const* __restrict__ faces, uint32_t n, uint32_t q)
{
	__shared__ float of_u8[256];
	const uint32_t v = threadIdx.y*CFENV_WG_X + threadIdx.x;
	cf_fill_of_u8(of_u8, v, type == CFHIP_PIXEL_RGBA8);
	__syncthreads();
	const uint32_t x = blockIdx.x*CFENV_WG_X + threadIdx.x, y = blockIdx.y*CFENV_WG_Y + threadIdx.y, f = blockIdx.z;
	if (x >= n || y >= n)
		return;
	const double dn = (double)n, dq = (double)q, dW = (double)W, dH = (double)H;
	double acc[4] = {0.0, 0.0, 0.0, 0.0};
	for (uint32_t b = 0; b < q; ++b)
		for (uint32_t a = 0; a < q; ++a) {
			double dx, dy, dz;
			face_dir(f, unit_coord((double)x + ((double)a + 0.5)/dq, dn), unit_coord((double)y + ((double)b + 0.5)/dq, dn), dx, dy, dz);
			const double m = (dx*dx + dy*dy) + dz*dz;
			const double phi = atan2(dx, dz), psi = asin(dy/sqrt(m));
			const double u = (phi/(2.0*CFENV_PI) + 0.5)*dW - 0.5, w = (0.5 - psi/CFENV_PI)*dH - 0.5;
			double x0f, y0f;
			const int32_t x0 = floor_index(u, -1, (int32_t)W - 1, &x0f), y0 = floor_index(w, -1, (int32_t)H - 1, &y0f);
			const double fx = u - x0f, fy = w - y0f, gx = 1.0 - fx, gy = 1.0 - fy;
			const uint32_t xa = x0 < 0 ? (uint32_t)(x0 + (int32_t)W) : (uint32_t)x0;
			const uint32_t xb = x0 + 1 >= (int32_t)W ? (uint32_t)(x0 + 1 - (int32_t)W) : (uint32_t)(x0 + 1);
			const uint32_t ya = (uint32_t)max(y0, 0), yb = (uint32_t)min(y0 + 1, (int32_t)H - 1);
			const uint8_t* r0 = src + (size_t)ya*pitch;
			const uint8_t* r1 = src + (size_t)yb*pitch;
			double c00[4], c10[4], c01[4], c11[4];
			panorama_texel(r0, xa, type, of_u8, c00);
			panorama_texel(r0, xb, type, of_u8, c10);
			panorama_texel(r1, xa, type, of_u8, c01);
			panorama_texel(r1, xb, type, of_u8, c11);
#pragma unroll
			for (int ch = 0; ch < 4; ++ch)
				acc[ch] = acc[ch] + (((c00[ch]*gx + c10[ch]*fx)*gy) + ((c01[ch]*gx + c11[ch]*fx)*fy));
		}
	const double qq = (double)(q*q);
	float4 out;
	out.x = (float)(acc[0]/qq); out.y = (float)(acc[1]/qq); out.z = (float)(acc[2]/qq); out.w = (float)(acc[3]/qq);
	static_cast<float4*>(faces[f])[(size_t)y*n + x] = out;
}

// ---- part 2 -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG)
cfhip_cube_prefilter_kernel(cfenv_prefilter_call c)
{
	__shared__ cfhip_ggx_sample tab[CFENV_CHUNK];
	__shared__ const float4* lvl[6u*CFENV_MAX_LEVELS];
	const uint32_t lane = threadIdx.x, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
	const uint32_t tid = wave*CFENV_WG_X + lane, L = c.src_levels;
	if (tid < 6u*L)
		lvl[tid] = static_cast<const float4*>(c.src[tid]);
	const uint32_t n = max(1u, c.face_size >> c.level);
	const uint64_t total = 6ull*n*n;
	uint64_t texel = (uint64_t)blockIdx.x*CFENV_WG_Y + wave;
	const bool live = texel < total;                   // a wavefront past the end works on the last texel and stores nothing
	if (!live)
		texel = total - 1u;
	const uint32_t f = (uint32_t)(texel/((uint64_t)n*n)), rem = (uint32_t)(texel%((uint64_t)n*n)), y = rem/n, x = rem%n;
	const double dn = (double)n;
	double nx, ny, nz;
	face_dir(f, unit_coord((double)x + 0.5, dn), unit_coord((double)y + 0.5, dn), nx, ny, nz);
	{
		const double r = sqrt((nx*nx + ny*ny) + nz*nz);
		nx = nx/r; ny = ny/r; nz = nz/r;
	}
	// the frame: up = (0, 0, 1) where |nz| < 0.999, else (1, 0, 0); tx = normalise(up x n), ty = n x tx
	const bool far = fabs(nz) < 0.999;
	double ax = far ? -ny : 0.0, ay = far ? nx : -nz, az = far ? 0.0 : ny;
	{
		const double r = sqrt((ax*ax + ay*ay) + az*az);
		ax = ax/r; ay = ay/r; az = az/r;
	}
	const double bx = ny*az - nz*ay, by = nz*ax - nx*az, bz = nx*ay - ny*ax;
	double acc[4] = {0.0, 0.0, 0.0, 0.0}, weight = 0.0;
	for (uint32_t base = 0; base < c.samples; base += CFENV_CHUNK) {
		const uint32_t count = min(CFENV_CHUNK, c.samples - base);
		__syncthreads();                               // the chunk before is read; the first time, the pointers are written
		for (uint32_t i = tid; i < count; i += WG)
			tab[i] = c.table[base + i];
		__syncthreads();
		for (uint32_t i = lane; i < count; i += CFENV_WG_X) {
			const cfhip_ggx_sample rec = tab[i];
			const double lx = (double)rec.lx, ly = (double)rec.ly, lz = (double)rec.lz;
			const double wx = (ax*lx + bx*ly) + nx*lz, wy = (ay*lx + by*ly) + ny*lz, wz = (az*lx + bz*ly) + nz*lz;
			uint32_t face;
			double s, t;
			dir_to_face(wx, wy, wz, face, s, t);
			// the table's lod is checked on the host: finite and within [0, CFENV_MAX_LEVELS]
			const uint32_t whole = (uint32_t)(int32_t)rec.lod;
			const uint32_t l0 = min(whole, L - 1u), l1 = min(l0 + 1u, L - 1u);
			const double g = (double)rec.lod - (double)whole;
			double c0[4], c1[4];
			fetch(lvl + l0, L, max(1u, c.face_size >> l0), face, s, t, c0);
			if (l1 != l0)
				fetch(lvl + l1, L, max(1u, c.face_size >> l1), face, s, t, c1);
#pragma unroll
			for (int ch = 0; ch < 4; ++ch) {
				const double second = l1 != l0 ? c1[ch] : c0[ch];
				acc[ch] = acc[ch] + (c0[ch]*(1.0 - g) + second*g)*lz;
			}
			weight = weight + lz;
		}
	}
	weight = butterfly(weight);
#pragma unroll
	for (int ch = 0; ch < 4; ++ch)
		acc[ch] = butterfly(acc[ch]);
	if (live && lane == 0) {
		float4 out;
		out.x = (float)(acc[0]/weight); out.y = (float)(acc[1]/weight); out.z = (float)(acc[2]/weight); out.w = (float)(acc[3]/weight);
		static_cast<float4*>(c.dst[f*c.dst_levels + c.level])[rem] = out;
	}
}

__global__ void __launch_bounds__(WG)
cfhip_cube_copy_kernel(cfenv_prefilter_call c)
{
	const uint32_t n = max(1u, c.face_size >> c.level), f = blockIdx.y;
	const uint64_t at = (uint64_t)blockIdx.x*WG + threadIdx.y*CFENV_WG_X + threadIdx.x;
	if (at < (uint64_t)n*n)
		static_cast<float4*>(c.dst[f*c.dst_levels + c.level])[at] = static_cast<const float4*>(c.src[f*c.src_levels + c.level])[at];
}

// ---- part 3 -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CFENV_WG_X)
cfhip_cube_sh9_rows_kernel(const void* const* __restrict__ faces, uint32_t n, double* __restrict__ rows)
{
	const uint32_t lane = threadIdx.x, y = blockIdx.x, f = blockIdx.y;
	const float4* __restrict__ row = static_cast<const float4*>(faces[f]) + (size_t)y*n;
	const double dn = (double)n, t = unit_coord((double)y + 0.5, dn), texel = 4.0/(dn*dn);
	double acc[CFENV_SH_VALUES];
#pragma unroll
	for (uint32_t k = 0; k < CFENV_SH_VALUES; ++k)
		acc[k] = 0.0;
	for (uint32_t x = lane; x < n; x += CFENV_WG_X) {      // the padding of a row adds 0.0: nothing
		const double s = unit_coord((double)x + 0.5, dn);
		const double r = (1.0 + s*s) + t*t, dw = texel/(r*sqrt(r));
		double dx, dy, dz;
		face_dir(f, s, t, dx, dy, dz);
		const double len = sqrt((dx*dx + dy*dy) + dz*dz);
		dx = dx/len; dy = dy/len; dz = dz/len;
		const double basis[9] = {CFENV_SH_C0, CFENV_SH_C1*dy, CFENV_SH_C1*dz, CFENV_SH_C1*dx, CFENV_SH_C2*(dx*dy),
			CFENV_SH_C2*(dy*dz), CFENV_SH_C20*(3.0*(dz*dz) - 1.0), CFENV_SH_C2*(dx*dz), CFENV_SH_C22*(dx*dx - dy*dy)};
		const float4 c = row[x];
#pragma unroll
		for (uint32_t b = 0; b < 9u; ++b) {
			const double w = basis[b]*dw;
			acc[4u*b] = acc[4u*b] + (double)c.x*w;
			acc[4u*b + 1u] = acc[4u*b + 1u] + (double)c.y*w;
			acc[4u*b + 2u] = acc[4u*b + 2u] + (double)c.z*w;
			acc[4u*b + 3u] = acc[4u*b + 3u] + (double)c.w*w;
		}
		acc[36] = acc[36] + dw;
	}
	double* __restrict__ out = rows + ((size_t)f*n + y)*CFENV_SH_VALUES;
#pragma unroll
	for (uint32_t k = 0; k < CFENV_SH_VALUES; ++k) {
		const double p = butterfly(acc[k]);
		if (lane == 0)
			out[k] = p;
	}
}

__global__ void __launch_bounds__(CFENV_WG_X)
cfhip_cube_sh9_final_kernel(const double* __restrict__ rows, uint32_t n, cfhip_sh9_result* __restrict__ result)
{
	__shared__ double omega;
	const uint32_t v = threadIdx.x;
	double sum = 0.0;
	if (v < CFENV_SH_VALUES)
		for (uint32_t r = 0; r < 6u*n; ++r)                // (face, y) order
			sum = sum + rows[(size_t)r*CFENV_SH_VALUES + v];
	if (v == 36u)
		omega = sum;
	__syncthreads();
	double* out = reinterpret_cast<double*>(result);
	if (v < 36u)
		out[v] = sum*((4.0*CFENV_PI)/omega);
	else if (v == 36u)
		out[v] = sum;
}

// ---- part 4: the BRDF lookup table -------------------------------------------------------------
// One wavefront per texel, four per workgroup, as the prefilter: lane j takes the records i = j mod 64 of the Hammersley
// table, staged in LDS CFENV_CHUNK at a time, and the lanes' sums meet in sum64's butterfly.  A wavefront past the end
// works on the last texel and stores nothing.  SHEEN: the Charlie column too -- the only pow in this file.
template <bool SHEEN>
__global__ void __launch_bounds__(WG)
cfhip_brdf_lut_kernel(float4* __restrict__ dst, uint32_t width, uint32_t height, const cfhip_hammersley_sample* __restrict__ table,
	uint32_t samples)
{
	__shared__ cfhip_hammersley_sample tab[CFENV_CHUNK];
	const uint32_t lane = threadIdx.x, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.y);
	const uint32_t tid = wave*CFENV_WG_X + lane, total = width*height;
	uint32_t texel = blockIdx.x*CFENV_WG_Y + wave;
	const bool live = texel < total;
	if (!live)
		texel = total - 1u;
	const uint32_t y = texel/width, x = texel%width;
	const double NoV = ((double)x + 0.5)/(double)width, r = ((double)y + 0.5)/(double)height;
	const double alpha = r*r, a2 = alpha*alpha;
	const double vx = sqrt(1.0 - NoV*NoV), vz = NoV;
	const double gv = sqrt((NoV*NoV)*(1.0 - a2) + a2);     // the view's half of the visibility term
	const double inv_alpha = 1.0/alpha, lead = 2.0 + inv_alpha;
	double A = 0.0, B = 0.0, C = 0.0;
	for (uint32_t base = 0; base < samples; base += CFENV_CHUNK) {
		const uint32_t count = min(CFENV_CHUNK, samples - base);
		__syncthreads();                               // the chunk before is read
		for (uint32_t i = tid; i < count; i += WG)
			tab[i] = table[base + i];
		__syncthreads();
		for (uint32_t i = lane; i < count; i += CFENV_WG_X) {
			const cfhip_hammersley_sample rec = tab[i];
			const double cphi = (double)rec.cos_phi, xi = (double)rec.xi1;
			{
				const double c2 = (1.0 - xi)/(1.0 + (a2 - 1.0)*xi);
				const double hz = sqrt(c2), st = sqrt(1.0 - c2), hx = st*cphi;
				const double VoH = (vx*hx) + (vz*hz), NoL = (2.0*VoH)*hz - vz;
				if (NoL > 0.0 && VoH > 0.0) {
					const double vis = 0.5/(NoL*gv + NoV*sqrt((NoL*NoL)*(1.0 - a2) + a2));
					const double t = ((vis*VoH)*NoL)/hz, m = 1.0 - VoH, fc = ((m*m)*(m*m))*m;
					A = A + (1.0 - fc)*t;
					B = B + fc*t;
				}
			}
			if (SHEEN) {
				const double hz = 1.0 - xi, st = sqrt(1.0 - hz*hz), hx = st*cphi;
				const double VoH = (vx*hx) + (vz*hz), NoL = (2.0*VoH)*hz - vz;
				if (NoL > 0.0 && VoH > 0.0) {
					const double vn = 1.0/(4.0*((NoL + NoV) - NoL*NoV));
					const double d = (lead*pow(st, inv_alpha))/(2.0*CFENV_PI);
					C = C + ((vn*d)*NoL)*VoH;
				}
			}
		}
	}
	A = butterfly(A);
	B = butterfly(B);
	if (SHEEN)
		C = butterfly(C);
	if (live && lane == 0) {
		const double S = (double)samples;
		float4 out;
		out.x = (float)((4.0*A)/S); out.y = (float)((4.0*B)/S); out.z = SHEEN ? (float)(((8.0*CFENV_PI)*C)/S) : 0.0f; out.w = 1.0f;
		dst[texel] = out;
	}
}

// ---- part 5: the irradiance cube from the nine coefficients --------------------------------------------------------------
// one texel per lane, the six faces in grid z; the 36 coefficients are the same for every lane: scalar loads
__global__ void __launch_bounds__(WG)
cfhip_cube_irradiance_kernel(const cfhip_sh9_result* __restrict__ sh, void* const* __restrict__ faces, uint32_t n, uint32_t over_pi)
{
	const uint32_t x = blockIdx.x*CFENV_WG_X + threadIdx.x, y = blockIdx.y*CFENV_WG_Y + threadIdx.y, f = blockIdx.z;
	if (x >= n || y >= n)
		return;
	const double dn = (double)n;
	double dx, dy, dz;
	face_dir(f, unit_coord((double)x + 0.5, dn), unit_coord((double)y + 0.5, dn), dx, dy, dz);
	const double len = sqrt((dx*dx + dy*dy) + dz*dz);
	dx = dx/len; dy = dy/len; dz = dz/len;
	const double basis[9] = {CFENV_SH_C0, CFENV_SH_C1*dy, CFENV_SH_C1*dz, CFENV_SH_C1*dx, CFENV_SH_C2*(dx*dy),
		CFENV_SH_C2*(dy*dz), CFENV_SH_C20*(3.0*(dz*dz) - 1.0), CFENV_SH_C2*(dx*dz), CFENV_SH_C22*(dx*dx - dy*dy)};
	// the cosine lobe's factor of each band: pi, 2 pi / 3, pi / 4
	constexpr double b1 = (2.0*CFENV_PI)/3.0, b2 = CFENV_PI/4.0;
	constexpr double band[9] = {CFENV_PI, b1, b1, b1, b2, b2, b2, b2, b2};
	double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
	for (uint32_t b = 0; b < 9u; ++b) {
		const double w = band[b]*basis[b];
#pragma unroll
		for (uint32_t ch = 0; ch < 4u; ++ch)
			acc[ch] = acc[ch] + w*sh->coeff[b][ch];
	}
	if (over_pi) {
#pragma unroll
		for (uint32_t ch = 0; ch < 4u; ++ch)
			acc[ch] = acc[ch]/CFENV_PI;
	}
	float4 out;
	out.x = (float)acc[0]; out.y = (float)acc[1]; out.z = (float)acc[2]; out.w = (float)acc[3];
	static_cast<float4*>(faces[f])[(size_t)y*n + x] = out;
}

} // namespace

extern "C" hipError_t cfhip_launch_brdf_lut(void* dst, uint32_t width, uint32_t height, const cfhip_hammersley_sample* table,
	uint32_t samples, uint32_t sheen, hipStream_t stream)
{
	const dim3 grid((width*height + CFENV_WG_Y - 1u)/CFENV_WG_Y), block(CFENV_WG_X, CFENV_WG_Y);
	if (sheen)
		hipLaunchKernelGGL(cfhip_brdf_lut_kernel<true>, grid, block, 0, stream, static_cast<float4*>(dst), width, height, table, samples);
	else
		hipLaunchKernelGGL(cfhip_brdf_lut_kernel<false>, grid, block, 0, stream, static_cast<float4*>(dst), width, height, table, samples);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_cube_irradiance(const cfhip_sh9_result* sh, void* const* faces, uint32_t face_size,
	uint32_t over_pi, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_cube_irradiance_kernel, dim3((face_size + CFENV_WG_X - 1u)/CFENV_WG_X,
		(face_size + CFENV_WG_Y - 1u)/CFENV_WG_Y, 6), dim3(CFENV_WG_X, CFENV_WG_Y), 0, stream, sh, faces, face_size, over_pi);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_equirect_to_cube(const void* src, int32_t src_type, uint32_t width, uint32_t height,
	unsigned long long src_pitch, void* const* faces, uint32_t face_size, uint32_t supersample, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_equirect_to_cube_kernel, dim3((face_size + CFENV_WG_X - 1u)/CFENV_WG_X,
		(face_size + CFENV_WG_Y - 1u)/CFENV_WG_Y, 6), dim3(CFENV_WG_X, CFENV_WG_Y), 0, stream, static_cast<const uint8_t*>(src),
		src_type, width, height, src_pitch, faces, face_size, supersample);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_cube_prefilter(const cfenv_prefilter_call* call, hipStream_t stream)
{
	const uint32_t n = call->face_size >> call->level ? call->face_size >> call->level : 1u;
	const uint64_t texels = (uint64_t)n*n;
	if (call->samples)
		hipLaunchKernelGGL(cfhip_cube_prefilter_kernel, dim3((uint32_t)((6u*texels + CFENV_WG_Y - 1u)/CFENV_WG_Y)),
			dim3(CFENV_WG_X, CFENV_WG_Y), 0, stream, *call);
	else
		hipLaunchKernelGGL(cfhip_cube_copy_kernel, dim3((uint32_t)((texels + WG - 1u)/WG), 6), dim3(CFENV_WG_X, CFENV_WG_Y), 0,
			stream, *call);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_cube_sh9_rows(const void* const* faces, uint32_t face_size, double* rows, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_cube_sh9_rows_kernel, dim3(face_size, 6), dim3(CFENV_WG_X), 0, stream, faces, face_size, rows);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_cube_sh9_final(const double* rows, uint32_t face_size, cfhip_sh9_result* result,
	hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_cube_sh9_final_kernel, dim3(1), dim3(CFENV_WG_X), 0, stream, rows, face_size, result);
	return hipGetLastError();
}
