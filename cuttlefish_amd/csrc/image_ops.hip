// image_ops.hip -- the per-image pixel operations of cuttlefish::Image (lib/src/Image.cpp:1513-1882) that the
// cuttlefish tool runs between loading an image and Texture::setImage (tool/main.cpp:164-276), fused into one
// pass: colour-space change, rotation, grayscale, normal map, X / Y flips, swizzle, alpha premultiplication, in
// that order.  Every op reads the RGBAF image as doubles and stores float (getPixelImpl /
// setPixelNoGrayscaleImpl), and each one rounds here exactly where the reference stores, so one launch is
// bit-identical to the same ops launched one at a time.
//
// Shape: a 256-thread workgroup owns a 32 x 32 tile of the ROTATED image.  It reads
// the matching source region with adjacent lanes on adjacent source texels of a row (16 B per lane for
// RGBA32F), transforms each texel once (colour change, then grayscale) and writes it into LDS at its rotated
// position, so a 90-degree rotation is an LDS transpose and not 64 source rows per wave instruction.  With the
// normal map on, the LDS tile holds the red channel only, with a 1-texel halo from the neighbouring tiles (or
// the opposite edge under wrap).  Each thread then forms 4 output texels from LDS -- normal, swizzle,
// premultiply -- and stores each as one float4 at its flipped position: a mirrored row is still one
// contiguous run of 512 B, written in reversed lane order.
// No kernel here may use scratch, spill a vector register or use AGPRs (cuttlefish_amd/build.py).
#include "cf_texel.h"

namespace {

constexpr uint32_t IT = 32;            // tile edge, in texels of the rotated image
constexpr uint32_t TS = IT + 1;        // float4 row stride of the colour tile: one slot of padding per row
constexpr uint32_t RS = IT + 3;        // float row stride of the red tile with its halo (IT + 2 texels, + 1 pad)

struct image_ops_args {
	const uint8_t* src;
	uint8_t* dst;
	unsigned long long pitch, dst_pitch;
	uint32_t w, h;                      // source size
	uint32_t rw, rh;                    // rotated (= output) size
	uint32_t ops;
	int src_srgb, dst_srgb;
	int rot;                            // quarter turns counter-clockwise: the k of np.rot90
	uint32_t normal_options;
	int rgbf;
	double height;
	int swz[4];
};

// a position of the rotated image outside it: the opposite edge under wrap, the edge texel itself otherwise
__device__ __forceinline__ uint32_t fold(int v, uint32_t n, bool wrap)
{
	if (v >= 0 && (uint32_t)v < n)
		return (uint32_t)v;
	if (wrap)
		return (uint32_t)cf_floor_mod(v, n);
	return v < 0 ? 0u : n - 1u;
}

__device__ __forceinline__ float channel(const float4& v, int c, float none)
{
	return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : c == 3 ? v.w : none;
}

template <int SRC_PIX>
__global__ void __launch_bounds__(256)
cfhip_image_ops_kernel(const image_ops_args a)
{
	__shared__ float4 tile[IT*TS];                    // colour tile; the normal map reuses it as the red tile
	__shared__ double lin_of_u8[SRC_PIX == 0 ? 256 : 1];
	const uint32_t ops = a.ops;
	const bool change = (ops & CFHIP_IMAGE_OP_COLOR_SPACE) && a.src_srgb != a.dst_srgb;
	const bool srgb = (ops & CFHIP_IMAGE_OP_COLOR_SPACE) ? a.dst_srgb : a.src_srgb;   // the space after the change
	const bool gray = ops & CFHIP_IMAGE_OP_GRAYSCALE;
	const bool normal = ops & CFHIP_IMAGE_OP_NORMAL_MAP;
	const bool wrap_x = normal && (a.normal_options & CFHIP_NORMAL_WRAP_X);
	const bool wrap_y = normal && (a.normal_options & CFHIP_NORMAL_WRAP_Y);
	const bool rgbf = a.rgbf || normal;
	// An 8-bit source has 256 possible sRGB values: their linear values are computed once per workgroup (the
	// same function on the same input as the per-texel call).  Only for the first op that linearises the
	// unmodified value, and kept in double: grayscale uses the linear value without a float store between -- which is
	// why the texel below is not cf_load_linear's: that one reads a float table and rounds where the mip chain stores.
	const bool lut = SRC_PIX == 0 && (change ? !a.dst_srgb : (gray && srgb));
	if (lut) {
		lin_of_u8[threadIdx.x] = cf_linear_of_u8(threadIdx.x);
		__syncthreads();
	}

	// ---- phase 1: the source region of the tile (plus the halo) -> LDS at its rotated position
	const uint32_t halo = normal ? 1u : 0u, E = IT + 2u*halo;
	const int rx0 = (int)(blockIdx.x*IT) - (int)halo, ry0 = (int)(blockIdx.y*IT) - (int)halo;
	float* red = reinterpret_cast<float*>(tile);
	for (uint32_t i = threadIdx.x; i < E*E; i += 256u) {
		// adjacent lanes take adjacent SOURCE x: along the rotated x for 0 / 180 degrees, along y for 90 / 270
		const uint32_t fast = i % E, slow = i/E;
		const uint32_t lx = (a.rot & 1) ? slow : fast, ly = (a.rot & 1) ? fast : slow;
		const uint32_t px = fold(rx0 + (int)lx, a.rw, wrap_x), py = fold(ry0 + (int)ly, a.rh, wrap_y);
		uint32_t sx = px, sy = py;                    // np.rot90(src, rot)[py][px] = src[sy][sx]
		if (a.rot == 1) {
			sx = a.w - 1u - py; sy = px;
		} else if (a.rot == 2) {
			sx = a.w - 1u - px; sy = a.h - 1u - py;
		} else if (a.rot == 3) {
			sx = py; sy = a.h - 1u - px;
		}
		const uint8_t* row = a.src + (size_t)sy*a.pitch;
		float4 p = load_rgbaf<SRC_PIX>(row, sx);
		const uint32_t u = SRC_PIX == 0 ? *reinterpret_cast<const uint32_t*>(row + (size_t)sx*4u) : 0u;
		if (a.rgbf)
			p.w = 1.0f;
		if (change) {                                 // Image::changeColorSpace
			if (a.dst_srgb) {
				p.x = (float)linear_to_srgb((double)p.x);
				p.y = (float)linear_to_srgb((double)p.y);
				p.z = (float)linear_to_srgb((double)p.z);
			} else if (lut) {
				p.x = (float)lin_of_u8[u & 255u];
				p.y = (float)lin_of_u8[(u >> 8) & 255u];
				p.z = (float)lin_of_u8[(u >> 16) & 255u];
			} else {
				p.x = (float)srgb_to_linear((double)p.x);
				p.y = (float)srgb_to_linear((double)p.y);
				p.z = (float)srgb_to_linear((double)p.z);
			}
		}
		if (gray) {                                   // Image::grayscale, in linear space
			double r = p.x, g = p.y, b = p.z;
			if (srgb && lut) {
				r = lin_of_u8[u & 255u];
				g = lin_of_u8[(u >> 8) & 255u];
				b = lin_of_u8[(u >> 16) & 255u];
			} else if (srgb) {
				r = srgb_to_linear(r);
				g = srgb_to_linear(g);
				b = srgb_to_linear(b);
			}
			double y = r*0.2126 + g*0.7152 + b*0.0722;   // toGrayscale (Color.h:213-217)
			if (srgb)
				y = linear_to_srgb(y);
			p.x = p.y = p.z = (float)y;
		}
		if (normal)
			red[ly*RS + lx] = p.x;
		else
			tile[ly*TS + lx] = p;
	}
	__syncthreads();

	// ---- phase 2: one output texel per thread and row step
	const bool keep_sign = a.normal_options & CFHIP_NORMAL_KEEP_SIGN;
	const bool flip_x = ops & CFHIP_IMAGE_OP_FLIP_X, flip_y = ops & CFHIP_IMAGE_OP_FLIP_Y;
	const uint32_t lx = threadIdx.x & (IT - 1u);
	const uint32_t px = blockIdx.x*IT + lx;
	for (uint32_t ly = threadIdx.x/IT; ly < IT; ly += 256u/IT) {
		const uint32_t py = blockIdx.y*IT + ly;
		if (px >= a.rw || py >= a.rh)
			continue;
		float4 v;
		if (normal) {                                 // Image::createNormalMap (Image.cpp:1783-1880)
			const float* c = red + (ly + 1u)*RS + (lx + 1u);
			const double dist_x = (!wrap_x && (px == 0 || px == a.rw - 1u)) ? 1.0 : 2.0;
			const double dist_y = (!wrap_y && (py == 0 || py == a.rh - 1u)) ? 1.0 : 2.0;
			const double dx = ((double)c[-1] - (double)c[1])*a.height/dist_x;
			const double dy = ((double)c[RS] - (double)c[-(int)RS])*a.height/dist_y;
			const double len = sqrt(dx*dx + dy*dy + 1);
			double nx = dx/len, ny = dy/len, nz = 1.0/len;
			if (!keep_sign) {
				nx = nx*0.5 + 0.5;
				ny = ny*0.5 + 0.5;
				nz = nz*0.5 + 0.5;
			}
			v = make_float4((float)nx, (float)ny, (float)nz, 1.0f);
		} else {
			v = tile[ly*TS + lx];
		}
		if (ops & CFHIP_IMAGE_OP_SWIZZLE) {          // every output reads the pre-swizzle texel
			const float4 s = v;
			v.x = channel(s, a.swz[0], 0.0f);
			v.y = channel(s, a.swz[1], 0.0f);
			v.z = channel(s, a.swz[2], 0.0f);
			v.w = rgbf ? 1.0f : channel(s, a.swz[3], 1.0f);
		}
		if ((ops & CFHIP_IMAGE_OP_PREMULTIPLY) && !rgbf) {   // no RGBF case in preMultiplyAlpha's switch
			double r = v.x, g = v.y, b = v.z;
			const double al = v.w;
			if (srgb) {
				r = srgb_to_linear(r);
				g = srgb_to_linear(g);
				b = srgb_to_linear(b);
			}
			r *= al;
			g *= al;
			b *= al;
			if (srgb) {
				r = linear_to_srgb(r);
				g = linear_to_srgb(g);
				b = linear_to_srgb(b);
			}
			v.x = (float)r;
			v.y = (float)g;
			v.z = (float)b;
		}
		const uint32_t ox = flip_x ? a.rw - 1u - px : px, oy = flip_y ? a.rh - 1u - py : py;
		*reinterpret_cast<float4*>(a.dst + (size_t)oy*a.dst_pitch + (size_t)ox*16u) = v;
	}
}

} // namespace

// The arguments were checked by cfhip_image_ops_device: sizes > 0 and below 2^20, enums in range, pitches
// covering a row, pointers aligned to their texel loads.
extern "C" hipError_t cfhip_launch_image_ops(const void* src, int src_pixel_type, size_t pitch, uint32_t w,
	uint32_t h, const cfhip_image_ops* o, void* dst, size_t dst_pitch, hipStream_t stream)
{
	image_ops_args a;
	a.src = static_cast<const uint8_t*>(src);
	a.dst = static_cast<uint8_t*>(dst);
	a.pitch = pitch;
	a.dst_pitch = dst_pitch;
	a.w = w;
	a.h = h;
	a.ops = o->ops;
	a.rot = 0;
	if (o->ops & CFHIP_IMAGE_OP_ROTATE) {
		static const int quarter_turns[6] = {3, 2, 1, 1, 2, 3};   // CW90, CW180, CW270, CCW90, CCW180, CCW270
		a.rot = quarter_turns[o->rotate];
	}
	a.rw = (a.rot & 1) ? h : w;
	a.rh = (a.rot & 1) ? w : h;
	a.src_srgb = o->src_color_space == CFHIP_COLOR_SRGB;
	a.dst_srgb = o->dst_color_space == CFHIP_COLOR_SRGB;
	a.normal_options = o->normal_options;
	a.rgbf = o->rgbf ? 1 : 0;
	a.height = o->normal_height;
	for (int c = 0; c < 4; ++c)
		a.swz[c] = o->swizzle[c];
	const dim3 grid((a.rw + IT - 1u)/IT, (a.rh + IT - 1u)/IT, 1), block(256, 1, 1);
	cf_pixel_dispatch(src_pixel_type, [&](auto pix) {
		hipLaunchKernelGGL(cfhip_image_ops_kernel<decltype(pix)::value>, grid, block, 0, stream, a);
	});
	return hipGetLastError();
}
