// pvrtc.hip -- PVRTC1 4 bpp (Texture::Format PVRTC1_RGB_4BPP = 59, PVRTC1_RGBA_4BPP = 60) on gfx950: the encoder's
// passes and the decoder, with a fused per-channel SSE.  CPU twin: tests/pvrtc_ref.py (same passes, same integer
// arithmetic; the GPU payload is byte-identical to it).  DESIGN.md section 4.10.
//
// The format, as Imagination publishes it (the PowerVR SDK's PVRTDecompress; the Khronos Data Format
// Specification, PVRTC section): 8-byte blocks, the 32-bit modulation word first (2 bits per texel, texel (x, y) at
// bit 2*(4y + x)), then the 32-bit colour word (bit 0 mode, bits 1-15 colour A, bits 16-31 colour B, bits 15 / 31
// their opaque flags).  A and B of a texel are the bilinear blend of the four blocks whose centres (texel 4b + 2)
// surround it, with wrap-around; mode 0 modulates by 0, 3, 5, 8 eighths, mode 1 ("punch-through") by 0, 4, 4, 8 and
// makes value 2 transparent.  Blocks are stored in twiddled (Morton) order, y in the lower bit of each pair.
//
// Encoder state (device scratch of the call): the RGBA8 texels of every surface (4 * bx by 4 * by, a surface under
// 8 px repeats itself), one colour word per block in raster order, one modulation byte per texel.  Bytes, not packed
// words: the blocks of one refine phase write different texels of the same neighbouring block.  Every pass is one
// launch over all surfaces of the call (the surface table; a uniform binary search finds a work item's surface), so
// a cube map with its mip tail costs what one surface costs in launches.
//
// Lane mapping: load and modulation -- 16 lanes per block, one per texel; init and pack -- one lane per block.
// Refine -- one wavefront per block: lanes 0..48 hold the 7 x 7 texels the block influences; the normal equations
// and the candidates' errors are wave sums.  Decode -- one lane per texel; its SSE form strides a bounded grid.
// -ffp-contract=off (build.py); every value that reaches the payload is integer arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cf_texel.h"
#include "pvrtc_surf.h"


namespace {

constexpr uint32_t kRidge = 64;            // pvrtc_ref.RIDGE
constexpr uint32_t kSwMode = 1, kSwCand = 2, kSwOpac = 4;

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the surface of work item `i` (blocks when phase == false, refine-phase blocks otherwise)
__device__ __forceinline__ uint32_t find_surf(const cf_pvrtc_surf* t, uint32_t n, uint32_t i, bool phase)
{
	uint32_t lo = 0, hi = n - 1;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1) >> 1;
		const uint32_t b = phase ? t[mid].ph_off : t[mid].blk_off;
		if (b <= i) lo = mid; else hi = mid - 1;
	}
	return lo;
}

struct Col { int r, g, b, a; };

// colour word -> A and B: RGB on the 5-bit scale, alpha on the 4-bit scale (pvrtc_ref.unpack)
__device__ __forceinline__ void unpack(uint32_t c, Col& A, Col& B)
{
	if (c & 0x8000u) {
		A.r = (c >> 10) & 31; A.g = (c >> 5) & 31; A.b = (c & 0x1e) | ((c & 0x1e) >> 4); A.a = 15;
	} else {
		A.r = ((c & 0xf00) >> 7) | ((c & 0xf00) >> 11); A.g = ((c & 0xf0) >> 3) | ((c & 0xf0) >> 7);
		A.b = ((c & 0xe) << 1) | ((c & 0xe) >> 2); A.a = (c & 0x7000) >> 11;
	}
	if (c & 0x80000000u) {
		B.r = (c >> 26) & 31; B.g = (c >> 21) & 31; B.b = (c >> 16) & 31; B.a = 15;
	} else {
		B.r = ((c & 0xf000000) >> 23) | ((c & 0xf000000) >> 27); B.g = ((c & 0xf00000) >> 19) | ((c & 0xf00000) >> 23);
		B.b = ((c & 0xf0000) >> 15) | ((c & 0xf0000) >> 19); B.a = (c & 0x70000000) >> 27;
	}
}

__device__ __forceinline__ void acc(Col& s, const Col& c, int w)
{
	s.r += w*c.r; s.g += w*c.g; s.b += w*c.b; s.a += w*c.a;
}

__device__ __forceinline__ Col to8(const Col& s)
{
	return Col{(s.r >> 6) + (s.r >> 1), (s.g >> 6) + (s.g >> 1), (s.b >> 6) + (s.b >> 1), (s.a >> 4) + s.a};
}

__device__ __forceinline__ int mod_weight(uint32_t mode, uint32_t m)
{
	return mode ? (m == 0 ? 0 : (m == 3 ? 8 : 4)) : (m == 0 ? 0 : (m == 1 ? 3 : (m == 2 ? 5 : 8)));
}

// decoded texel from 8-bit A and B (pvrtc_ref.blend); rgb: the RGB format, whose alpha is 255
__device__ __forceinline__ Col blend(const Col& A, const Col& B, uint32_t mode, uint32_t m, bool rgb)
{
	const int w = mod_weight(mode, m);
	Col o{(A.r*(8 - w) + B.r*w) >> 3, (A.g*(8 - w) + B.g*w) >> 3, (A.b*(8 - w) + B.b*w) >> 3,
		(A.a*(8 - w) + B.a*w) >> 3};
	if (rgb) o.a = 255;
	else if (mode && m == 2) o.a = 0;
	return o;
}

__device__ __forceinline__ uint32_t sq_err(const Col& o, uint32_t t, uint32_t wmask)
{
	const int dr = o.r - (int)(t & 255u), dg = o.g - (int)((t >> 8) & 255u), db = o.b - (int)((t >> 16) & 255u),
		da = o.a - (int)(t >> 24);
	return (wmask & 1u ? (uint32_t)(dr*dr) : 0u) + (wmask & 2u ? (uint32_t)(dg*dg) : 0u) +
		(wmask & 4u ? (uint32_t)(db*db) : 0u) + (wmask & 8u ? (uint32_t)(da*da) : 0u);
}

// first minimum over the four modulation values
__device__ __forceinline__ uint32_t best_mod(const Col& A, const Col& B, uint32_t t, uint32_t mode, uint32_t wmask,
	bool rgb, uint32_t* err)
{
	uint32_t bm = 0, be = 0xFFFFFFFFu;
	for (uint32_t m = 0; m < 4; ++m) {
		const uint32_t e = sq_err(blend(A, B, mode, m, rgb), t, wmask);
		if (e < be) { be = e; bm = m; }
	}
	*err = be;
	return bm;
}

// the four blocks of texel (px, py) and their weights, P Q R S (pvrtc_ref.texel_blocks); grid bx x by, powers of two
__device__ __forceinline__ void texel_blocks(uint32_t px, uint32_t py, uint32_t bx, uint32_t by, uint32_t idx[4],
	int wt[4])
{
	const int u = (int)((px + 2u) & 3u), v = (int)((py + 2u) & 3u);
	const uint32_t x0 = ((px + 4u*bx - 2u) >> 2) & (bx - 1u), y0 = ((py + 4u*by - 2u) >> 2) & (by - 1u);
	const uint32_t x1 = (x0 + 1u) & (bx - 1u), y1 = (y0 + 1u) & (by - 1u);
	idx[0] = y0*bx + x0; idx[1] = y0*bx + x1; idx[2] = y1*bx + x0; idx[3] = y1*bx + x1;
	wt[0] = (4 - u)*(4 - v); wt[1] = u*(4 - v); wt[2] = (4 - u)*v; wt[3] = u*v;
}

// bilinear sums of A and B at a texel from the call's colour words
__device__ __forceinline__ void texel_sums(const uint32_t* words, uint32_t px, uint32_t py, uint32_t bx, uint32_t by,
	Col& sa, Col& sb)
{
	uint32_t idx[4];
	int wt[4];
	texel_blocks(px, py, bx, by, idx, wt);
	sa = Col{0, 0, 0, 0}; sb = Col{0, 0, 0, 0};
	for (int k = 0; k < 4; ++k) {
		Col A, B;
		unpack(words[idx[k]], A, B);
		acc(sa, A, wt[k]);
		acc(sb, B, wt[k]);
	}
}

__device__ __forceinline__ uint32_t twiddle(uint32_t x, uint32_t y, uint32_t lbx, uint32_t lby)
{
	const uint32_t m = lbx < lby ? lbx : lby;
	uint32_t idx = 0;
	for (uint32_t i = 0; i < m; ++i)
		idx |= ((y >> i) & 1u) << (2u*i) | ((x >> i) & 1u) << (2u*i + 1u);
	if (lbx > m) idx |= (x >> m) << (2u*m);
	else if (lby > m) idx |= (y >> m) << (2u*m);
	return idx;
}

__device__ __forceinline__ uint32_t log2u(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

// (uint8)round(clamp(f, 0, 1) * 255), NaN -> 0: toColorBlock's quantisation (the host pipeline's host_unorm8)
__device__ __forceinline__ uint32_t unorm8(float f)
{
	if (!(f > 0.0f))
		return 0;
	f = f > 1.0f ? 1.0f : f;
	return (uint32_t)roundf(f*255.0f);
}

__device__ __forceinline__ uint32_t load_texel(const cf_pvrtc_surf& s, uint32_t x, uint32_t y)
{
	const uint8_t* row = s.src + (long long)y*s.pitch;
	if (s.pix == 0)
		return *reinterpret_cast<const uint32_t*>(row + (size_t)x*4u);
	float4 f;
	if (s.pix == 1)
		f = *reinterpret_cast<const float4*>(row + (size_t)x*16u);
	else
		f = cf_halves_to_float4(*reinterpret_cast<const uint2*>(row + (size_t)x*8u));
	return unorm8(f.x) | unorm8(f.y) << 8 | unorm8(f.z) << 16 | unorm8(f.w) << 24;
}

__device__ __forceinline__ uint32_t enc_a(const Col& c, bool opaque)
{
	if (opaque)
		return 0x8000u | (uint32_t)c.r << 10 | (uint32_t)c.g << 5 | (uint32_t)((c.b*15 + 15)/31) << 1;
	const uint32_t a3 = (uint32_t)min((c.a + 1) >> 1, 7);
	return a3 << 12 | (uint32_t)((c.r*15 + 15)/31) << 8 | (uint32_t)((c.g*15 + 15)/31) << 4 |
		(uint32_t)((c.b*7 + 15)/31) << 1;
}

__device__ __forceinline__ uint32_t enc_b(const Col& c, bool opaque)
{
	if (opaque)
		return 0x80000000u | (uint32_t)c.r << 26 | (uint32_t)c.g << 21 | (uint32_t)c.b << 16;
	const uint32_t a3 = (uint32_t)min((c.a + 1) >> 1, 7);
	return a3 << 28 | (uint32_t)((c.r*15 + 15)/31) << 24 | (uint32_t)((c.g*15 + 15)/31) << 20 |
		(uint32_t)((c.b*15 + 15)/31) << 16;
}

// candidate k (0..15) of the +-1 set (pvrtc_ref._step_field): colour k >> 3, field (k >> 1) & 3, up when k & 1
__device__ __forceinline__ uint32_t step_field(uint32_t word, uint32_t k)
{
	const uint32_t col = k >> 3, j = (k >> 1) & 3u, up = k & 1u;
	const bool opaque = (word >> (col ? 31 : 15)) & 1u;
	uint32_t sh, bits;
	if (col == 0 && opaque) {
		if (j >= 3) return word;
		sh = j == 0 ? 10 : (j == 1 ? 5 : 1); bits = j == 2 ? 4 : 5;
	} else if (col == 0) {
		sh = j == 0 ? 12 : (j == 1 ? 8 : (j == 2 ? 4 : 1)); bits = (j == 0 || j == 3) ? 3 : 4;
	} else if (opaque) {
		if (j >= 3) return word;
		sh = j == 0 ? 26 : (j == 1 ? 21 : 16); bits = 5;
	} else {
		sh = j == 0 ? 28 : (j == 1 ? 24 : (j == 2 ? 20 : 16)); bits = j == 0 ? 3 : 4;
	}
	const uint32_t mask = (1u << bits) - 1u;
	const uint32_t v = (word >> sh) & mask;
	if (up ? v == mask : v == 0)
		return word;
	const uint32_t nv = up ? v + 1u : v - 1u;
	return (word & ~(mask << sh)) | nv << sh;
}

// floor((2n + d) / 2d) for d > 0 (pvrtc_ref._rdiv)
__device__ __forceinline__ long long rdiv(long long n, long long d)
{
	const long long a = 2*n + d, b = 2*d;
	long long q = a / b;
	if ((a % b != 0) && (a < 0)) --q;
	return q;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
	for (int o = 32; o >= 1; o >>= 1)
		v += (uint32_t)__shfl_xor((int)v, o, 64);
	return v;
}

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
	for (int o = 32; o >= 1; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

} // namespace

// ---- load: the sources of all surfaces -> RGBA8 texels (16 lanes per block) ----
__global__ __launch_bounds__(256) void cfhip_pvrtc_load_kernel(const cf_pvrtc_surf* tab, uint32_t n,
	uint32_t total_blocks, uint32_t* tex)
{
	const uint32_t g = blockIdx.x*256u + threadIdx.x;
	const uint32_t blk = g >> 4;
	if (blk >= total_blocks)
		return;
	const cf_pvrtc_surf s = tab[find_surf(tab, n, blk, false)];
	const uint32_t lb = blk - s.blk_off, i = g & 15u;
	const uint32_t px = (lb % s.bx)*4u + (i & 3u), py = (lb / s.bx)*4u + (i >> 2);
	tex[16u*s.blk_off + py*4u*s.bx + px] = load_texel(s, px & (s.w - 1u), py & (s.h - 1u));
}

// ---- init: A = per-channel minimum, B = maximum of each block's texels (pvrtc_ref.init_words) ----
__global__ __launch_bounds__(256) void cfhip_pvrtc_init_kernel(const cf_pvrtc_surf* tab, uint32_t n,
	uint32_t total_blocks, const uint32_t* tex, uint32_t* words, int rgb)
{
	const uint32_t blk = blockIdx.x*256u + threadIdx.x;
	if (blk >= total_blocks)
		return;
	const cf_pvrtc_surf s = tab[find_surf(tab, n, blk, false)];
	const uint32_t lb = blk - s.blk_off;
	const uint32_t pw = 4u*s.bx;
	const uint32_t* t0 = tex + 16u*s.blk_off + (lb / s.bx)*4u*pw + (lb % s.bx)*4u;
	int lo[4] = {255, 255, 255, 255}, hi[4] = {0, 0, 0, 0};
	for (uint32_t y = 0; y < 4; ++y)
		for (uint32_t x = 0; x < 4; ++x) {
			const uint32_t t = t0[y*pw + x];
			for (int c = 0; c < 4; ++c) {
				const int v = (int)((t >> (8*c)) & 255u);
				lo[c] = min(lo[c], v); hi[c] = max(hi[c], v);
			}
		}
	const Col ca{(lo[0]*31 + 127)/255, (lo[1]*31 + 127)/255, (lo[2]*31 + 127)/255, (lo[3]*15 + 127)/255};
	const Col cb{(hi[0]*31 + 127)/255, (hi[1]*31 + 127)/255, (hi[2]*31 + 127)/255, (hi[3]*15 + 127)/255};
	words[blk] = enc_a(ca, rgb || ca.a == 15) | enc_b(cb, rgb || cb.a == 15);
}

// ---- modulation: every texel's exact argmin; RGBA blocks pick their mode (pvrtc_ref.modulation_pass) ----
// A block's lanes rewrite bit 0 of its own colour word while neighbouring blocks read that word: they read bits
// 1-31 only, which no lane changes, so either value of the word gives them the same colours.
__global__ __launch_bounds__(256) void cfhip_pvrtc_mod_kernel(const cf_pvrtc_surf* tab, uint32_t n,
	uint32_t total_blocks, const uint32_t* tex, uint32_t* words, uint8_t* mods, uint32_t wmask, int rgb)
{
	const uint32_t g = blockIdx.x*256u + threadIdx.x;
	const uint32_t blk = g >> 4;
	const bool act = blk < total_blocks;
	uint32_t e0 = 0, e1 = 0, m0 = 0, m1 = 0, ti = 0;
	if (act) {
		const cf_pvrtc_surf s = tab[find_surf(tab, n, blk, false)];
		const uint32_t lb = blk - s.blk_off, i = g & 15u;
		const uint32_t px = (lb % s.bx)*4u + (i & 3u), py = (lb / s.bx)*4u + (i >> 2);
		ti = 16u*s.blk_off + py*4u*s.bx + px;
		Col sa, sb;
		texel_sums(words + s.blk_off, px, py, s.bx, s.by, sa, sb);
		const Col A = to8(sa), B = to8(sb);
		const uint32_t t = tex[ti];
		m0 = best_mod(A, B, t, 0, wmask, rgb != 0, &e0);
		if (!rgb)
			m1 = best_mod(A, B, t, 1, wmask, false, &e1);
	}
	// the 16 lanes of a block are 16 consecutive lanes of the wavefront
	for (int o = 8; o >= 1; o >>= 1) {
		e0 += (uint32_t)__shfl_xor((int)e0, o, 16);
		e1 += (uint32_t)__shfl_xor((int)e1, o, 16);
	}
	if (!act)
		return;
	const bool pt = !rgb && e1 < e0;
	mods[ti] = (uint8_t)(pt ? m1 : m0);
	if ((threadIdx.x & 15u) == 0)
		words[blk] = (words[blk] & ~1u) | (pt ? 1u : 0u);
}

// ---- refine: one parity phase, a wavefront per block (pvrtc_ref.refine_phase) ----
__global__ __launch_bounds__(256) void cfhip_pvrtc_refine_kernel(const cf_pvrtc_surf* tab, uint32_t n,
	uint32_t phase_blocks, const uint32_t* tex, uint32_t* words, uint8_t* mods, uint32_t wmask, int rgb, uint32_t ox,
	uint32_t oy, uint32_t flags)
{
	const uint32_t wv = rfl(blockIdx.x*4u + (threadIdx.x >> 6));
	if (wv >= phase_blocks)
		return;
	const cf_pvrtc_surf s = tab[find_surf(tab, n, wv, true)];
	const uint32_t li = wv - s.ph_off, hb = s.bx >> 1;
	const uint32_t cx = ox + 2u*(li % hb), cy = oy + 2u*(li / hb);
	const uint32_t pw = 4u*s.bx, ph = 4u*s.by;
	uint32_t* W = words + s.blk_off;
	const uint32_t* T = tex + 16u*s.blk_off;
	uint8_t* M = mods + 16u*s.blk_off;
	const uint32_t cword = W[cy*s.bx + cx];
	Col Ac, Bc;
	unpack(cword, Ac, Bc);

	uint32_t lane = threadIdx.x & 63u;
	const bool act = lane < 49u;
	const uint32_t di = act ? lane % 7u : 0u, dj = act ? lane / 7u : 0u;
	const uint32_t px = (4u*cx + pw - 1u + di) & (pw - 1u), py = (4u*cy + ph - 1u + dj) & (ph - 1u);
	const int hx = di < 4u ? (int)di + 1 : 7 - (int)di, hy = dj < 4u ? (int)dj + 1 : 7 - (int)dj;
	const int wP = act ? hx*hy : 0;
	const bool own = di >= 1u && di <= 4u && dj >= 1u && dj <= 4u;
	const uint32_t t = T[py*pw + px];
	Col sa, sb;
	texel_sums(W, px, py, s.bx, s.by, sa, sb);
	const uint32_t nb_mode = W[(py >> 2)*s.bx + (px >> 2)] & 1u;
	const uint32_t m_cur = M[py*pw + px];
	// the region's error as it stands
	uint32_t e_old = sq_err(blend(to8(sa), to8(sb), nb_mode, m_cur, rgb != 0), t, wmask);
	const uint32_t old = wave_sum_u32(act ? e_old : 0u);
	// the neighbours' part of the sums
	const Col ra{sa.r - wP*Ac.r, sa.g - wP*Ac.g, sa.b - wP*Ac.b, sa.a - wP*Ac.a};
	const Col rb{sb.r - wP*Bc.r, sb.g - wP*Bc.g, sb.b - wP*Bc.b, sb.a - wP*Bc.a};

	// least squares for the centre's A and B, the current modulation held
	const int w = mod_weight(nb_mode, m_cur);
	const int al = (8 - w)*wP, be = w*wP;
	const bool pt = nb_mode && m_cur == 2u;
	const int ala = pt ? 0 : al, bea = pt ? 0 : be;
	const long long saa = (long long)wave_sum_u32((uint32_t)(al*al)) + kRidge;
	const long long sbb = (long long)wave_sum_u32((uint32_t)(be*be)) + kRidge;
	const long long sab = (long long)wave_sum_u32((uint32_t)(al*be));
	const long long saa_a = (long long)wave_sum_u32((uint32_t)(ala*ala)) + kRidge;
	const long long sbb_a = (long long)wave_sum_u32((uint32_t)(bea*bea)) + kRidge;
	const long long sab_a = (long long)wave_sum_u32((uint32_t)(ala*bea));
	Col solA, solB;
	for (int ch = 0; ch < 4; ++ch) {
		const int rac = ch == 0 ? ra.r : (ch == 1 ? ra.g : (ch == 2 ? ra.b : ra.a));
		const int rbc = ch == 0 ? rb.r : (ch == 1 ? rb.g : (ch == 2 ? rb.b : rb.a));
		const int tc = (int)((t >> (8*ch)) & 255u);
		const long long fn = ch < 3 ? 255 : 17, fd = ch < 3 ? 31 : 1;
		const long long y = (long long)tc*128*fd - fn*(long long)((8 - w)*rac + w*rbc);
		const int a_ = ch < 3 ? al : ala, b_ = ch < 3 ? be : bea;
		const int acur = ch == 0 ? Ac.r : (ch == 1 ? Ac.g : (ch == 2 ? Ac.b : Ac.a));
		const int bcur = ch == 0 ? Bc.r : (ch == 1 ? Bc.g : (ch == 2 ? Bc.b : Bc.a));
		const long long say = wave_sum_i64(act ? (long long)a_*y : 0) + (long long)kRidge*fn*acur;
		const long long sby = wave_sum_i64(act ? (long long)b_*y : 0) + (long long)kRidge*fn*bcur;
		const long long Saa = ch < 3 ? saa : saa_a, Sbb = ch < 3 ? sbb : sbb_a, Sab = ch < 3 ? sab : sab_a;
		const long long det = Saa*Sbb - Sab*Sab;
		const long long top = ch < 3 ? 31 : 15;
		long long va = rdiv(Sbb*say - Sab*sby, fn*det), vb = rdiv(Saa*sby - Sab*say, fn*det);
		va = va < 0 ? 0 : (va > top ? top : va);
		vb = vb < 0 ? 0 : (vb > top ? top : vb);
		if (ch == 0) { solA.r = (int)va; solB.r = (int)vb; }
		else if (ch == 1) { solA.g = (int)va; solB.g = (int)vb; }
		else if (ch == 2) { solA.b = (int)va; solB.b = (int)vb; }
		else { solA.a = (int)va; solB.a = (int)vb; }
	}
	if (rgb)
		flags &= ~(kSwMode | kSwOpac);
	const bool opa = rgb || solA.a == 15, opb = rgb || solB.a == 15;
	const uint32_t mode_c = cword & 1u;
	const uint32_t base = rfl(enc_a(solA, opa) | enc_b(solB, opb) | mode_c);
	const uint32_t ncand = 1u + ((flags & kSwCand) ? 16u : 0u) + ((flags & kSwMode) ? 1u : 0u) +
		((flags & kSwOpac) ? 3u : 0u);

	// candidate k in pvrtc_ref's order: base, +-1 steps, mode flip, opacity flips
	uint32_t best_s = 0xFFFFFFFFu, best_w = base;
	for (uint32_t k = 0; k < ncand; ++k) {
		uint32_t cw = base, r = k;
		if (r > 0) {
			--r;
			if (flags & kSwCand) {
				if (r < 16u) cw = step_field(base, r);
				r = r < 16u ? 0xFFFFFFFFu : r - 16u;
			}
			if (r != 0xFFFFFFFFu && (flags & kSwMode)) {
				if (r == 0u) cw = base ^ 1u;
				r = r == 0u ? 0xFFFFFFFFu : r - 1u;
			}
			if (r != 0xFFFFFFFFu)   // opacity flips (only with kSwOpac, which counts them)
				cw = enc_a(solA, r == 1u ? opa : !opa) | enc_b(solB, r == 0u ? opb : !opb) | mode_c;
		}
		cw = rfl(cw);
		Col ca, cb;
		unpack(cw, ca, cb);
		Col xa = ra, xb = rb;
		acc(xa, ca, wP);
		acc(xb, cb, wP);
		uint32_t e;
		best_mod(to8(xa), to8(xb), t, own ? (cw & 1u) : nb_mode, wmask, rgb != 0, &e);
		const uint32_t ssum = wave_sum_u32(act ? e : 0u);
		if (ssum < best_s) { best_s = ssum; best_w = cw; }
	}
	if (best_s > old)
		return;
	Col ca, cb;
	unpack(best_w, ca, cb);
	Col xa = ra, xb = rb;
	acc(xa, ca, wP);
	acc(xb, cb, wP);
	uint32_t e;
	const uint32_t m = best_mod(to8(xa), to8(xb), t, own ? (best_w & 1u) : nb_mode, wmask, rgb != 0, &e);
	lane = threadIdx.x & 63u;
	if (lane < 49u)
		M[py*pw + px] = (uint8_t)m;
	if (lane == 0u)
		W[cy*s.bx + cx] = best_w;
}

// ---- pack: modulation bytes + colour words -> twiddled 64-bit blocks ----
__global__ __launch_bounds__(256) void cfhip_pvrtc_pack_kernel(const cf_pvrtc_surf* tab, uint32_t n,
	uint32_t total_blocks, const uint32_t* words, const uint8_t* mods)
{
	const uint32_t blk = blockIdx.x*256u + threadIdx.x;
	if (blk >= total_blocks)
		return;
	const cf_pvrtc_surf s = tab[find_surf(tab, n, blk, false)];
	const uint32_t lb = blk - s.blk_off, bxi = lb % s.bx, byi = lb / s.bx, pw = 4u*s.bx;
	const uint8_t* m0 = mods + 16u*s.blk_off + byi*4u*pw + bxi*4u;
	uint32_t mw = 0;
	for (uint32_t y = 0; y < 4; ++y)
		for (uint32_t x = 0; x < 4; ++x)
			mw |= ((uint32_t)m0[y*pw + x] & 3u) << (2u*(4u*y + x));
	const unsigned long long v = (unsigned long long)mw | (unsigned long long)words[blk] << 32;
	const uint32_t idx = twiddle(bxi, byi, log2u(s.bx), log2u(s.by));
	uint8_t* o = s.out + (size_t)idx*8u;
	if (((uintptr_t)o & 7u) == 0)
		*reinterpret_cast<unsigned long long*>(o) = v;
	else
		for (int b = 0; b < 8; ++b)
			o[b] = (uint8_t)(v >> (8*b));
}

// ---- decode: one lane per texel; SSE: per-channel sums against an RGBA8 reference instead of texels ----
// The SSE form runs a bounded grid that strides over the texels and sums per lane, per wavefront and then per
// workgroup in LDS: four 64-bit atomics per workgroup, not per wavefront (a million waves adding into the same four
// words serialise on them).
__device__ __forceinline__ void decode_texel(const uint8_t* blocks, uint32_t px, uint32_t py, uint32_t bx,
	uint32_t by, uint32_t lbx, uint32_t lby, int rgb, Col& o)
{
	uint32_t idx[4];
	int wt[4];
	texel_blocks(px, py, bx, by, idx, wt);
	Col sa{0, 0, 0, 0}, sb{0, 0, 0, 0};
	for (int k = 0; k < 4; ++k) {
		const uint32_t tw = twiddle(idx[k] & (bx - 1u), idx[k] >> lbx, lbx, lby);
		Col A, B;
		unpack(*reinterpret_cast<const uint32_t*>(blocks + (size_t)tw*8u + 4u), A, B);
		acc(sa, A, wt[k]);
		acc(sb, B, wt[k]);
	}
	const uint8_t* own = blocks + (size_t)twiddle(px >> 2, py >> 2, lbx, lby)*8u;
	const uint32_t mw = *reinterpret_cast<const uint32_t*>(own);
	const uint32_t cw = *reinterpret_cast<const uint32_t*>(own + 4u);
	o = blend(to8(sa), to8(sb), cw & 1u, (mw >> (2u*(4u*(py & 3u) + (px & 3u)))) & 3u, rgb != 0);
}

__global__ __launch_bounds__(256) void cfhip_pvrtc_decode_kernel(const uint8_t* blocks, uint32_t w, uint32_t h,
	int rgb, uint8_t* out, size_t out_pitch)
{
	const uint32_t g = blockIdx.x*256u + threadIdx.x;
	if (g >= w*h)
		return;
	const uint32_t bx = w/4u > 2u ? w/4u : 2u, by = h/4u > 2u ? h/4u : 2u;
	const uint32_t px = g & (w - 1u), py = g >> log2u(w);
	Col o;
	decode_texel(blocks, px, py, bx, by, log2u(bx), log2u(by), rgb, o);
	*reinterpret_cast<uint32_t*>(out + (size_t)py*out_pitch + (size_t)px*4u) =
		(uint32_t)o.r | (uint32_t)o.g << 8 | (uint32_t)o.b << 16 | (uint32_t)o.a << 24;
}

__global__ __launch_bounds__(256) void cfhip_pvrtc_decode_sse_kernel(const uint8_t* blocks, uint32_t w, uint32_t h,
	int rgb, const uint8_t* ref, size_t ref_pitch, unsigned long long* sums)
{
	__shared__ unsigned long long part[4][4];
	const uint32_t texels = w*h;
	const uint32_t bx = w/4u > 2u ? w/4u : 2u, by = h/4u > 2u ? h/4u : 2u;
	const uint32_t lbx = log2u(bx), lby = log2u(by), lw = log2u(w);
	unsigned long long d[4] = {0, 0, 0, 0};
	for (uint32_t g = blockIdx.x*256u + threadIdx.x; g < texels; g += gridDim.x*256u) {
		const uint32_t px = g & (w - 1u), py = g >> lw;
		Col o;
		decode_texel(blocks, px, py, bx, by, lbx, lby, rgb, o);
		const uint32_t r = *reinterpret_cast<const uint32_t*>(ref + (size_t)py*ref_pitch + (size_t)px*4u);
		const int dr = o.r - (int)(r & 255u), dg = o.g - (int)((r >> 8) & 255u), db = o.b - (int)((r >> 16) & 255u),
			da = o.a - (int)(r >> 24);
		d[0] += (uint32_t)(dr*dr); d[1] += (uint32_t)(dg*dg); d[2] += (uint32_t)(db*db); d[3] += (uint32_t)(da*da);
	}
	for (int c = 0; c < 4; ++c)
		d[c] = (unsigned long long)wave_sum_i64((long long)d[c]);
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (lane == 0)
		for (int c = 0; c < 4; ++c)
			part[wave][c] = d[c];
	__syncthreads();
	if (threadIdx.x < 4u) {
		const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
			part[3][threadIdx.x];
		if (v)
			atomicAdd(&sums[threadIdx.x], v);
	}
}

// ---- host-side launchers (cfhip_api.hip) ----
extern "C" hipError_t cfhip_pvrtc_launch(int pass, const cf_pvrtc_surf* tab, uint32_t n, uint32_t items,
	uint32_t* tex, uint32_t* words, uint8_t* mods, uint32_t wmask, int rgb, uint32_t ox, uint32_t oy, uint32_t flags,
	hipStream_t stream)
{
	if (!items)
		return hipSuccess;
	switch (pass) {
		case 0:
			hipLaunchKernelGGL(cfhip_pvrtc_load_kernel, dim3((items + 15u)/16u), dim3(256), 0, stream, tab, n, items, tex);
			break;
		case 1:
			hipLaunchKernelGGL(cfhip_pvrtc_init_kernel, dim3((items + 255u)/256u), dim3(256), 0, stream, tab, n, items,
				tex, words, rgb);
			break;
		case 2:
			hipLaunchKernelGGL(cfhip_pvrtc_mod_kernel, dim3((items + 15u)/16u), dim3(256), 0, stream, tab, n, items,
				tex, words, mods, wmask, rgb);
			break;
		case 3:
			hipLaunchKernelGGL(cfhip_pvrtc_refine_kernel, dim3((items + 3u)/4u), dim3(256), 0, stream, tab, n, items,
				tex, words, mods, wmask, rgb, ox, oy, flags);
			break;
		default:
			hipLaunchKernelGGL(cfhip_pvrtc_pack_kernel, dim3((items + 255u)/256u), dim3(256), 0, stream, tab, n, items,
				words, mods);
			break;
	}
	return hipGetLastError();
}

extern "C" hipError_t cfhip_pvrtc_launch_decode(const void* blocks, uint32_t w, uint32_t h, int rgb, void* out,
	size_t out_pitch, const void* ref, size_t ref_pitch, unsigned long long* sums, int sse, hipStream_t stream)
{
	const uint32_t wgs = (w*h + 255u)/256u;
	if (sse)
		hipLaunchKernelGGL(cfhip_pvrtc_decode_sse_kernel, dim3(wgs < 4096u ? wgs : 4096u), dim3(256), 0, stream,
			static_cast<const uint8_t*>(blocks), w, h, rgb, static_cast<const uint8_t*>(ref), ref_pitch, sums);
	else
		hipLaunchKernelGGL(cfhip_pvrtc_decode_kernel, dim3(wgs), dim3(256), 0, stream,
			static_cast<const uint8_t*>(blocks), w, h, rgb, static_cast<uint8_t*>(out), out_pitch);
	return hipGetLastError();
}
