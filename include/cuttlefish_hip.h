/*
 * cuttlefish_hip.h -- C ABI of the MI355X-native block-texture encoder backend.
 *
 * This is the drop-in boundary for the ONE hot path of Cuttlefish:
 *
 *   Texture::convert            lib/src/Texture.cpp:1536-1561
 *     -> Converter::convert     lib/src/Converter.cpp:508-593   (per-surface job loop)
 *       -> createConverter      lib/src/Converter.cpp:32-506    (BC: :339-412)
 *         -> S3tcConverter::process / compressBlock
 *                               lib/src/S3tcConverter.cpp:242-255, :263-646
 *
 * The reference has no FFI for this path (converters are compiled-in C++
 * subclasses of cuttlefish::Converter, lib/src/Converter.h:31-76).  The binding a
 * maintainer adds is a whole-surface Converter subclass (jobsX()==jobsY()==1, the
 * PvrtcConverter pattern, lib/src/PvrtcConverter.h:37-38) that forwards to
 * cfhip_encode(); see INTEGRATION.md and integration/cuttlefish/HipConverter.cpp.
 *
 * Plain C: pointers, sizes, ints.  No C++/torch types cross this boundary.  All
 * entry points are thread-safe per context, never throw and never abort; errors
 * are negative CFHIP_E_* codes with cfhip_last_error() text.  There is NO CPU
 * fallback inside this library: with no HIP device cfhip_create() fails.
 */
#ifndef CUTTLEFISH_HIP_H
#define CUTTLEFISH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFHIP_ABI_VERSION 1

/* Values mirror cuttlefish::Texture::Format (lib/include/cuttlefish/Texture.h:59-130). */
enum cfhip_format {
	/* Uncompressed ("standard") formats: one output pixel per source pixel, row-major, tightly
	 * packed; cfhip_query answers block 1x1 and the bytes per pixel.  Replaces the
	 * StandardConverter family (lib/src/StandardConverter.h:44-515, StandardConverter.cpp:22-467)
	 * with the (format, type) legality of createConverter (lib/src/Converter.cpp:38-337).
	 * quality / alpha / mask / color_space are ignored, as the reference's converters ignore them.
	 * NaN converts to 0 and float -> integer conversions saturate (undefined in the reference). */
	CFHIP_FORMAT_R4G4 = 1,
	CFHIP_FORMAT_R4G4B4A4 = 2,
	CFHIP_FORMAT_B4G4R4A4 = 3,
	CFHIP_FORMAT_A4R4G4B4 = 4,
	CFHIP_FORMAT_R5G6B5 = 5,
	CFHIP_FORMAT_B5G6R5 = 6,
	CFHIP_FORMAT_R5G5B5A1 = 7,
	CFHIP_FORMAT_B5G5R5A1 = 8,
	CFHIP_FORMAT_A1R5G5B5 = 9,
	CFHIP_FORMAT_R8 = 10,
	CFHIP_FORMAT_R8G8 = 11,
	CFHIP_FORMAT_R8G8B8 = 12,
	CFHIP_FORMAT_B8G8R8 = 13,
	CFHIP_FORMAT_R8G8B8A8 = 14,
	CFHIP_FORMAT_B8G8R8A8 = 15,
	CFHIP_FORMAT_A8B8G8R8 = 16,
	CFHIP_FORMAT_A2R10G10B10 = 17,
	CFHIP_FORMAT_A2B10G10R10 = 18,
	CFHIP_FORMAT_R16 = 19,
	CFHIP_FORMAT_R16G16 = 20,
	CFHIP_FORMAT_R16G16B16 = 21,
	CFHIP_FORMAT_R16G16B16A16 = 22,
	CFHIP_FORMAT_R32 = 23,
	CFHIP_FORMAT_R32G32 = 24,
	CFHIP_FORMAT_R32G32B32 = 25,
	CFHIP_FORMAT_R32G32B32A32 = 26,
	CFHIP_FORMAT_B10G11R11_UFLOAT = 27,
	CFHIP_FORMAT_E5B9G9R9_UFLOAT = 28,
	/* Block-compressed formats. */
	CFHIP_FORMAT_BC1_RGB = 29,
	CFHIP_FORMAT_BC1_RGBA = 30,
	CFHIP_FORMAT_BC2 = 31,
	CFHIP_FORMAT_BC3 = 32,
	CFHIP_FORMAT_BC4 = 33,
	CFHIP_FORMAT_BC5 = 34,
	CFHIP_FORMAT_BC6H = 35,
	CFHIP_FORMAT_BC7 = 36,
	CFHIP_FORMAT_ETC1 = 37,
	CFHIP_FORMAT_ETC2_R8G8B8 = 38,
	CFHIP_FORMAT_ETC2_R8G8B8A1 = 39,
	CFHIP_FORMAT_ETC2_R8G8B8A8 = 40,
	CFHIP_FORMAT_EAC_R11 = 41,
	CFHIP_FORMAT_EAC_R11G11 = 42,
	CFHIP_FORMAT_ASTC_4x4 = 43,
	CFHIP_FORMAT_ASTC_5x4 = 44,
	CFHIP_FORMAT_ASTC_5x5 = 45,
	CFHIP_FORMAT_ASTC_6x5 = 46,
	CFHIP_FORMAT_ASTC_6x6 = 47,
	CFHIP_FORMAT_ASTC_8x5 = 48,
	CFHIP_FORMAT_ASTC_8x6 = 49,
	CFHIP_FORMAT_ASTC_8x8 = 50,
	CFHIP_FORMAT_ASTC_10x5 = 51,
	CFHIP_FORMAT_ASTC_10x6 = 52,
	CFHIP_FORMAT_ASTC_10x8 = 53,
	CFHIP_FORMAT_ASTC_10x10 = 54,
	CFHIP_FORMAT_ASTC_12x10 = 55,
	CFHIP_FORMAT_ASTC_12x12 = 56,
	/* PVRTC (Texture.h:124-129).  cfhip_query, cfhip_encode*, cfhip_decode*, cfhip_decoded_layout and
	 * cfhip_compare* answer CFHIP_E_UNSUPPORTED for all six: PVRTC1 4 bpp has the cfhip_pvrtc_* entries below;
	 * the 2 bpp and PVRTC2 formats are not built. */
	CFHIP_FORMAT_PVRTC1_RGB_2BPP = 57,
	CFHIP_FORMAT_PVRTC1_RGBA_2BPP = 58,
	CFHIP_FORMAT_PVRTC1_RGB_4BPP = 59,
	CFHIP_FORMAT_PVRTC1_RGBA_4BPP = 60,
	CFHIP_FORMAT_PVRTC2_RGBA_2BPP = 61,
	CFHIP_FORMAT_PVRTC2_RGBA_4BPP = 62
};

/* cuttlefish::Texture::Type (Texture.h:135-143) */
enum cfhip_type {
	CFHIP_TYPE_UNORM = 0,
	CFHIP_TYPE_SNORM = 1,
	CFHIP_TYPE_UINT = 2,
	CFHIP_TYPE_INT = 3,
	CFHIP_TYPE_UFLOAT = 4,
	CFHIP_TYPE_FLOAT = 5
};

/* cuttlefish::Texture::Quality (Texture.h:181-188) */
enum cfhip_quality {
	CFHIP_QUALITY_LOWEST = 0,
	CFHIP_QUALITY_LOW = 1,
	CFHIP_QUALITY_NORMAL = 2,
	CFHIP_QUALITY_HIGH = 3,
	CFHIP_QUALITY_HIGHEST = 4
};

/* cuttlefish::Texture::Alpha (Texture.h:161-167) */
enum cfhip_alpha {
	CFHIP_ALPHA_NONE = 0,
	CFHIP_ALPHA_STANDARD = 1,
	CFHIP_ALPHA_PREMULTIPLIED = 2,
	CFHIP_ALPHA_ENCODED = 3
};

/* cuttlefish::ColorSpace (lib/include/cuttlefish/Color.h:40-44) */
enum cfhip_color_space {
	CFHIP_COLOR_LINEAR = 0,
	CFHIP_COLOR_SRGB = 1
};

/* Source pixel layouts.  RGBA32F is the reference's ColorRGBAf scanline
 * (Converter.h:52-56 asserts Image::Format::RGBAF); RGBA8 is what toColorBlock
 * (S3tcConverter.cpp:97-111) produces from it and costs a quarter of the upload. */
enum cfhip_pixel_type {
	CFHIP_PIXEL_RGBA8 = 0,
	CFHIP_PIXEL_RGBA32F = 1,
	CFHIP_PIXEL_RGBA16F = 2
};

enum cfhip_error {
	CFHIP_OK = 0,
	CFHIP_E_INVALID = -1,      /* bad argument */
	CFHIP_E_UNSUPPORTED = -2,  /* (format, type) pair createConverter would reject / not built yet */
	CFHIP_E_CAPACITY = -3,     /* out_capacity too small */
	CFHIP_E_DEVICE = -4,       /* HIP runtime error (text in cfhip_last_error) */
	CFHIP_E_NO_DEVICE = -5,    /* no usable gfx950 device */
	CFHIP_E_DATA = -6          /* cfhip_inflate: the stream or its index is invalid (class and chunk in cfhip_last_error) */
};

typedef struct cfhip_ctx cfhip_ctx;

/* Conversion parameters = the arguments of Texture::convert (Texture.h:740-742)
 * plus the image colour space the converters read (S3tcConverter.cpp:233). */
typedef struct cfhip_params {
	int32_t format;       /* enum cfhip_format */
	int32_t type;         /* enum cfhip_type */
	int32_t quality;      /* enum cfhip_quality */
	int32_t alpha;        /* enum cfhip_alpha */
	uint8_t mask_rgba[4]; /* Texture::ColorMask r,g,b,a; non-zero = channel participates */
	int32_t color_space;  /* enum cfhip_color_space */
} cfhip_params;

/* One surface = one (mip, depth, face) image of Converter::convert's loop
 * (Converter.cpp:521-527).  pixels: top-down rows (Image::scanline order,
 * Image.cpp:340-343), row_pitch_bytes apart: `pixels` addresses row 0 and the pitch may be
 * NEGATIVE (the reference's FreeImage bitmaps are stored bottom-up, so a Converter can hand
 * over image.scanline(0) and scanline(1) - scanline(0) without touching a pixel).  out receives
 * ceil(w/bw)*ceil(h/bh)*block_bytes, blocks row-major (S3tcConverter.cpp:239,244).
 * Partial edge blocks replicate the last row/column (S3tcConverter.cpp:246-252). */
typedef struct cfhip_surface {
	const void* pixels;
	int32_t pixel_type;     /* enum cfhip_pixel_type */
	uint32_t width, height;
	ptrdiff_t row_pitch_bytes;
	void* out;
	size_t out_capacity;
} cfhip_surface;

int cfhip_abi_version(void);

/* Number of visible HIP devices (0 if none / runtime unavailable). */
int cfhip_device_count(void);

/* One context per GPU (one process per GPU in multi-GPU jobs).  NULL on failure;
 * *err (optional) receives the CFHIP_E_* code. */
cfhip_ctx* cfhip_create(int device_id, unsigned flags, int* err);
void cfhip_destroy(cfhip_ctx* ctx);

/* Block geometry of a format = Texture::blockWidth/blockHeight/blockSize
 * (Texture.cpp:529,611,693-773); CFHIP_E_UNSUPPORTED for illegal (format,type)
 * pairs exactly where createConverter returns nullptr (Converter.cpp:339-412). */
int cfhip_query(int format, int type, int* block_w, int* block_h, int* block_bytes);

/* Host-buffer entry point (what HipConverter::process calls): uploads each
 * surface, encodes on the GPU, downloads the payload.  Blocking. */
int cfhip_encode(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n_surfaces,
	const cfhip_params* params);
/* Several GPUs from ONE process (the reference's CLI and library are a single process; the
 * surfaces of a call are independent, Converter.cpp:521-589): the surfaces are assigned to the
 * contexts -- one per device -- by block count (longest-processing-time, SURVEY.md section 8e(i);
 * deterministic), and every context encodes its share with cfhip_encode on a host thread of its
 * own.  Same result as cfhip_encode(ctxs[0], ...) byte for byte; the first failure is returned
 * (its text through cfhip_last_error of that context) and the payload buffers are then
 * unspecified.  n_ctx == 1 is exactly cfhip_encode. */
int cfhip_encode_multi(cfhip_ctx* const* ctxs, int n_ctx, const cfhip_surface* surfaces,
	size_t n_surfaces, const cfhip_params* params);
/* The same with a release hook: Converter::convert frees every source image as soon as its surface is
 * converted (lib/src/Converter.cpp:586), so that a texture array with mip chains never holds all of its
 * RGBAF images and all of its payloads at once.  consumed(user, i) is called once the library has finished
 * READING surfaces[i].pixels -- the surface's last strip was gathered / quantised into the pipeline's pinned
 * memory, or the group of small surfaces it was uploaded with has left the host -- after which the caller may
 * free that source.  With several contexts the function runs on the contexts' worker threads, possibly for
 * different surfaces at the same time; it must not call into this library.  If the call FAILS after some
 * surfaces were reported, those sources are gone: the caller cannot re-run the work on another path for them
 * (HipConverter then fails the conversion, as a codec failure would).  Everything that can be checked is
 * checked before the first surface is read (parameters, sizes, capacities), so what is left to fail late are
 * HIP runtime errors.  consumed == NULL is exactly cfhip_encode_multi. */
typedef void (*cfhip_consumed_fn)(void* user, size_t surface_index);
int cfhip_encode_multi_ex(cfhip_ctx* const* ctxs, int n_ctx, const cfhip_surface* surfaces,
	size_t n_surfaces, const cfhip_params* params, cfhip_consumed_fn consumed, void* user);
/* Host pipeline of cfhip_encode: small surfaces of a call are
 * uploaded together and encoded in ONE batched launch with one synchronisation; a large
 * RGBA32F surface of an 8-bit format, or any bottom-up surface, is cut into strips of whole
 * block rows that host threads gather -- and quantise to UNORM8 with the arithmetic of
 * toColorBlock (S3tcConverter.cpp:97-111) -- into pinned memory while earlier strips upload and
 * encode.  The payload is byte-identical whichever way a surface travels. */

/* Device-buffer entry point: pixels/out of every surface are device pointers on
 * ctx's GPU (e.g. produced by a GPU mip generator).  Kernels are enqueued on
 * `stream` (a hipStream_t, NULL = the context's own stream) and the call returns
 * without synchronising when stream != NULL.  The context's own stream is NON-BLOCKING: it
 * does not order itself against the legacy default stream (handle 0, which is what NULL is read
 * as).  A caller whose producer ran on the default stream -- torch's current stream unless one
 * was set -- synchronises the device before a stream = NULL call, or passes a real stream. */
int cfhip_encode_device(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n_surfaces,
	const cfhip_params* params, void* stream);

/* Mip-chain generation on the GPU, feeding cfhip_encode_device
 * without a host round trip.  Stands in for Texture::generateMipmaps (lib/src/Texture.cpp:
 * 1320-1514, 2-D path :1442-1511): level k = Image::resize(level k-1, max(1, w >> k),
 * max(1, h >> k), filter) (lib/src/Image.cpp:1324-1511), resized in LINEAR space -- an sRGB
 * image is converted with sRGBToLinear, resized and converted back with linearToSRGB
 * (Image.cpp:1337-1346, Color.h:224-242; alpha is not converted) -- on RGBAF images whose
 * float storage rounds every intermediate.  Filters: in a stock build Image::resize hands all
 * five to FreeImage_Rescale (Image.cpp:1348-1380: Box -> FILTER_BOX, Linear -> FILTER_BILINEAR,
 * Cubic -> FILTER_BICUBIC, CatmullRom -- the reference's default -- and BSpline), a third-party
 * library that is absent: they run a restatement of FreeImage's published two-pass weights-table
 * resampler -- same results class, parity unpinned.  Box / Linear | CFHIP_FILTER_FALLBACK select
 * the arithmetic Image::resize runs itself when FreeImage_Rescale returns no image
 * (Image.cpp:1393-1447, :1448-1505), which IS in the reference tree.
 *   src / src_pixel_type / src_pitch_bytes : level 0 on the device (RGBA8 is read as v/255.0,
 *                                            RGBA16F / RGBA32F as stored)
 *   dst_levels[k-1], k = 1..levels-1       : device buffers that receive level k as tightly
 *                                            packed RGBA32F (16 B/texel), the reference's RGBAF
 * Kernels are enqueued on `stream` (NULL = the context's stream, then the call synchronises). */
enum cfhip_resize_filter {     /* Image::ResizeFilter (Image.h), same values */
	CFHIP_FILTER_BOX = 0,
	CFHIP_FILTER_LINEAR = 1,
	CFHIP_FILTER_CUBIC = 2,
	CFHIP_FILTER_CATMULL_ROM = 3,
	CFHIP_FILTER_BSPLINE = 4,
	CFHIP_FILTER_FALLBACK = 0x100  /* flag, Box / Linear only: the in-tree loops instead of FreeImage's */
};
int cfhip_generate_mips_device(cfhip_ctx* ctx, const void* src, int src_pixel_type,
	uint32_t width, uint32_t height, size_t src_pitch_bytes, int color_space, int filter,
	void* const* dst_levels, uint32_t levels, void* stream);

/* The same for the layers of an array or cube texture: Texture::generateMipmaps resizes every
 * [depth][face] image of a level on its own (lib/src/Texture.cpp:1442-1511 inside its loops over depth
 * and faces), so the `layers` surfaces -- all width x height, `src_pixel_type`, `src_pitch_bytes` -- are
 * independent chains.  They share one launch per pass and level (the small levels of a chain are a few
 * microseconds each: 256 chains one after the other are launch-bound, 5 632 launches against 22).
 *   srcs[l]                                  : level 0 of layer l on the device
 *   dst_levels[l*(levels-1) + (k-1)]         : receives level k of layer l (RGBA32F, tightly packed)
 * Results are bit-identical to `layers` calls of cfhip_generate_mips_device. */
int cfhip_generate_mips_array_device(cfhip_ctx* ctx, const void* const* srcs, uint32_t layers,
	int src_pixel_type, uint32_t width, uint32_t height, size_t src_pitch_bytes, int color_space,
	int filter, void* const* dst_levels, uint32_t levels, void* stream);

/* The repairs of a generated mip chain before it is encoded, on the chain where cfhip_generate_mips_array_device
 * left it (same srcs / levels layout; levels[] are modified in place, level 0 is only read).
 *
 * CFHIP_MIP_POST_COVERAGE: alpha-tested textures thin out level by level, because every filter averages alpha.  Each
 * level's alpha is scaled so that as many of its texels pass `alpha >= alpha_threshold` as of level 0's, in proportion.
 *   alpha(x)        level 0: RGBA8 (float)(v / 255.0), RGBA16F half -> float, RGBA32F as stored; levels: as stored
 *   count(L, s, t)  texels of L with fl32(alpha * s) >= t: one float32 multiply, one compare; NaN and negative alphas
 *                   never count; 0 < t <= 1; non-decreasing in s > 0
 *   C0, T_k         C0 = count(level 0, 1, t); T_k = (C0 * n_k + n_0 / 2) / n_0 in 64-bit integers, n = texels
 *   scale of level k, with S_MIN = 0.25f, S_MAX = 4.0f, c1 = count(level k, 1, t), prev / next the adjacent float32:
 *     1. c1 == T_k: s = 1
 *     2. c1 <  T_k: u = the smallest float32 in (1, S_MAX] with count >= T_k and d = prev(u); no such u: S_MAX alone
 *     3. c1 >  T_k: d = the largest float32 in [S_MIN, 1) with count <= T_k and u = next(d); no such d: S_MIN alone
 *     4. of two candidates the one whose count is nearer to T_k, a tie to u (the larger count)
 *     5. if the chosen candidate's count equals c1: s = 1
 *   applied         s != 1: alpha = fminf(fl32(alpha * s), 1.0f); s == 1: no byte of the level changes; RGB untouched
 * Premultiplied colour is out of scope: alpha alone is scaled, so run the pass on straight alpha.
 *
 * CFHIP_MIP_POST_NORMALIZE: every texel's RGB of every level renormalised, in double, alpha untouched.
 *   x = (double)c with CFHIP_MIP_POST_SIGNED_NORMALS, else (double)c * 2.0 - 1.0 (Image::createNormalMap's storage
 *   without KEEP_SIGN); len = sqrt((x*x + y*y) + z*z); len not finite or not > 0: the normal is (0, 0, 1), else x / len;
 *   stored as (float)x, or (float)(x * 0.5 + 0.5).
 * With both flags one pass over the levels applies both; the result equals the two flags in two calls.
 *
 *   results_device  layers * (levels_count - 1) records, [l * (levels_count - 1) + (k - 1)] for level k of layer l;
 *                   required with COVERAGE, ignored otherwise
 * All layers and levels share every launch: 15 with COVERAGE (1 gather, 7 decide, 6 count, 1 apply), 1 without, and
 * nothing inside the call waits for the host.  levels[] entries are 16-byte aligned.  levels_count: 2 to the chain's
 * length.  Every argument is checked before anything is enqueued; stream == NULL means the context's stream and the
 * call synchronises.  Identical calls return identical bytes. */
enum { CFHIP_MIP_POST_COVERAGE = 1, CFHIP_MIP_POST_NORMALIZE = 2, CFHIP_MIP_POST_SIGNED_NORMALS = 4 };
typedef struct cfhip_mip_post_params {
	uint32_t flags;
	float alpha_threshold;
} cfhip_mip_post_params;
typedef struct cfhip_mip_post_result {
	float scale;
	uint32_t target;
	uint32_t count_before;
	uint32_t count_after;
} cfhip_mip_post_result;
int cfhip_mip_post_array_device(cfhip_ctx* ctx, const void* const* srcs, uint32_t layers, int src_pixel_type,
	uint32_t width, uint32_t height, size_t src_pitch_bytes, void* const* levels, uint32_t levels_count,
	const cfhip_mip_post_params* params, cfhip_mip_post_result* results_device, void* stream);

/* The building block: counts_device[i] = count(surfaces[i], scale, threshold) as defined above, for `count` surfaces
 * of any sizes and pixel types in one launch (users measure the coverage of decoded payloads with it).  pixels and
 * pitch_bytes are aligned to a component of the pixel type; scale is positive and finite. */
typedef struct cfhip_coverage_surface {
	const void* pixels;
	int32_t pixel_type;
	uint32_t width;
	uint32_t height;
	size_t pitch_bytes;
} cfhip_coverage_surface;
int cfhip_alpha_coverage_device(cfhip_ctx* ctx, const cfhip_coverage_surface* surfaces, uint32_t count, float threshold,
	float scale, uint32_t* counts_device, void* stream);

/* Alpha bleeding (solidify, edge padding): before mips and encoding, every texel whose alpha is not above a threshold
 * takes the colour of the nearest texel whose alpha is.  Alpha is untouched, so the image looks the same, but filters
 * and block encoders see a sensible colour on both sides of a cut-out's silhouette instead of whatever the exporter left
 * there.  The remedy for straight alpha; premultiplied input is out of scope.  In place, on `layers` surfaces of one size
 * and pixel type: images[l] is width x height texels, 1 <= width, height <= 32768, rows pitch_bytes apart.
 *
 *   seed            texel p is a seed iff alpha(p) > alpha_threshold, 0 <= alpha_threshold < 1, compared in float32;
 *                   alpha() as the coverage pass reads it: RGBA8 (float)(v / 255.0), RGBA16F half -> float, RGBA32F as
 *                   stored.  A NaN alpha is not a seed.  Seed word: x | y << 16; 0xFFFFFFFF means none.
 *   distance        dx = |px - sx|, on a wrapped axis (CFHIP_BLEED_WRAP_X / _Y) dx = min(dx, width - dx); the same for
 *                   y; d^2 = dx^2 + dy^2 < 2^31.  The key of a candidate seed s for texel p is the 64-bit
 *                   d^2(p, s) << 32 | s: ties go to the smaller seed word.
 *   passes          P = the smallest power of two >= max(width, height); the steps are P/2, P/4, ..., 1 and one more 1
 *                   (a 1 x 1 surface: the one step 1).  Pass 0 writes each texel's own seed word, or none.  Each step k
 *                   reads only the buffer the pass before it wrote: texel p's candidates are the seeds stored at
 *                   p + k * (dx, dy), dx, dy in {-1, 0, 1}, p itself included; on a wrapped axis the position is taken
 *                   modulo the size, on an unwrapped axis a position outside the surface is skipped.  p keeps the
 *                   candidate of minimal key, or none; the minimum makes the order of the nine reads irrelevant.
 *   fill            after the last step every texel that is not a seed takes the R, G, B storage bits of its seed's
 *                   texel if it has a seed and max_distance == 0 (unlimited) or d^2 <= max_distance^2,
 *                   max_distance <= 65535.  No arithmetic: the bits are copied in the surface's own pixel type.  Alpha
 *                   and all seed texels are never written.  A surface without seeds is left untouched.
 *   results_device  one record per layer, or NULL for none: seeds, filled, max_dist2 (the largest d^2 among the filled
 *                   texels, 0 if none), reserved = 0.  Sums and a maximum: identical calls return identical bytes.
 * This is a jump flood, not an exact Euclidean transform: without wrap every texel receives a seed whenever the surface
 * has one (any offset below P is a sum of distinct steps, and the path stays inside the bounding box of seed and texel),
 * its seed is never nearer than the nearest one, and rarely farther (tests/test_alpha_bleed_ref.py bounds how often).
 *
 * All layers share every launch: 2 + log2(P) launches per call (seed, log2(P) steps, the last step fused with the fill),
 * plain launches on the call's stream, nothing waits for the host.  The scratch is the context's, grown on demand:
 * 8 bytes per texel of the call (two buffers of seed words), at most 2^31 texels per call.  images[l] and pitch_bytes
 * are aligned to a component of the pixel type.  Every argument is checked before anything is enqueued; stream == NULL
 * means the context's stream and the call synchronises. */
enum { CFHIP_BLEED_WRAP_X = 1, CFHIP_BLEED_WRAP_Y = 2 };
typedef struct cfhip_bleed_params {
	uint32_t flags;
	float alpha_threshold;
	uint32_t max_distance;
} cfhip_bleed_params;
typedef struct cfhip_bleed_result {
	uint32_t seeds;
	uint32_t filled;
	uint32_t max_dist2;
	uint32_t reserved;
} cfhip_bleed_result;
int cfhip_alpha_bleed_array_device(cfhip_ctx* ctx, void* const* images, uint32_t layers, int pixel_type,
	uint32_t width, uint32_t height, size_t pitch_bytes, const cfhip_bleed_params* params,
	cfhip_bleed_result* results_device, void* stream);

/* Signed distance field from alpha (Green, "Improved Alpha-Tested Magnification for Vector Textures and Special
 * Effects", 2007): a high-resolution cut-out is classified, every texel's distance to the silhouette is measured, and
 * the distance is stored at low resolution, scaled so that 0.5 is the edge.  Bilinear magnification then reconstructs a
 * clean edge from a texture 8 or 16 times smaller per side.  The third tool for straight-alpha cut-outs, beside the
 * coverage pass and alpha bleeding above.
 *
 *   input           `layers` source surfaces src[l] of one size width x height (1 to 32768 each) and one pixel type,
 *                   rows src_pitch_bytes apart, only read.  alpha() as the coverage and bleed passes read it: RGBA8
 *                   (float)(v / 255.0), RGBA16F half -> float, RGBA32F as stored.
 *   class           texel p is inside iff alpha(p) > alpha_threshold, compared in float32, 0 <= alpha_threshold < 1.
 *                   A NaN alpha is outside.
 *   distance        spread: an integer, 1 to 126, in source texels; K = spread + 1.  For texel p,
 *                   e(p) = min(K^2, min{dx^2 + dy^2 : q a texel of the other class}), dx = |px - qx|, on an axis wrapped
 *                   by CFHIP_SDF_WRAP_X / _Y dx = min(dx, width - dx); the same for y.  Outside an unwrapped surface
 *                   there are no texels; a surface of a single class has e = K^2 everywhere.  This is the true
 *                   Euclidean transform between texel centres, capped at K -- not a flood.
 *   signed distance rho(e) = (float)sqrt((double)e), both operations IEEE; sd(p) = rho - 0.5 inside, 0.5 - rho outside:
 *                   the silhouette lies half-way between two centres.  Every sd is a multiple of 2^-23 below 2^7, so a
 *                   double sum of up to 256 of them is exact in any order.
 *   output          scale s in {1, 2, 4, 8, 16}; width and height are multiples of s.  Output texel (X, Y) takes
 *                   m = (the sum of sd over its s x s source texels) / s^2 in double, which is exact, and
 *                   v = 0.5 + m / (2.0 * spread) in double, clamped to [0, 1].  With K = spread + 1 a tile farther than
 *                   the spread from the silhouette reaches exactly 0 or 1.
 *   store           dst[l] is width/s x height/s texels of dst_pixel_type, rows dst_pitch_bytes apart.  channel_mask
 *                   (bits R = 1, G = 2, B = 4, A = 8, not 0) names the components that receive v: RGBA8 takes
 *                   (uint8)floor(v * 255 + 0.5), RGBA32F (float)v, RGBA16F (float)v rounded to half, nearest-even.  The
 *                   other components are not written.  dst[l] may equal src[l] when s = 1 and the pixel types are
 *                   equal: all alpha is read before anything is written.
 *   results_device  one record per layer, or NULL for none: inside (source texels inside), saturated (source texels
 *                   with e == K^2), two reserved zeros.  Sums: identical calls return identical bytes.
 *
 * All layers share every launch: a classify pass (one bit per texel), a row pass (each texel's capped distance within
 * its row, from bit scans), a column pass (the windowed minimum of dy^2 + row distance^2, out of LDS) and, for s > 1, a
 * resolve pass; at s = 1 the column pass stores v itself.  3 or 4 plain launches per call whatever the layers, spread or
 * scale, on the call's stream; nothing waits for the host.  The scratch is the context's, grown on demand: per source
 * texel one byte (row pass), two more for s > 1 (e), and one bit (the classes, whole 64-bit words per row) -- within
 * 4 bytes per texel for widths from 8.  At most 2^31 source texels per call.  Pointers and pitches are aligned to a
 * component of their pixel type.  Every argument is checked before anything is enqueued; stream == NULL means the
 * context's stream and the call synchronises. */
enum { CFHIP_SDF_WRAP_X = 1, CFHIP_SDF_WRAP_Y = 2 };
typedef struct cfhip_sdf_params {
	uint32_t flags;
	float alpha_threshold;
	uint32_t spread;
	uint32_t scale;
	uint32_t channel_mask;
	uint32_t reserved;
} cfhip_sdf_params;
typedef struct cfhip_sdf_result {
	uint32_t inside;
	uint32_t saturated;
	uint32_t reserved[2];
} cfhip_sdf_result;
int cfhip_alpha_sdf_array_device(cfhip_ctx* ctx, const void* const* src, uint32_t layers, int src_pixel_type,
	uint32_t width, uint32_t height, size_t src_pitch_bytes, void* const* dst, int dst_pixel_type,
	size_t dst_pitch_bytes, const cfhip_sdf_params* params, cfhip_sdf_result* results_device, void* stream);

/* Specular anti-aliasing (Toksvig 2005; Han et al. 2007; Neubelt and Pettineo 2013; Kaplanyan et al. 2016): the levels
 * of a roughness chain take up the variance of the level-0 normals inside each texel's footprint -- what averaging and
 * renormalising a normal map discards -- so that a distant, bumpy surface renders rough instead of mirror-smooth.  Run
 * on the generated roughness (or packed ORM) chain before it is encoded.  One channel of levels 1... is overwritten:
 * the value written replaces the mip filter's own value in that channel (it is the footprint mean of alpha^2 plus the
 * variance, not a correction of the filter's result).  Level 0, the other three channels and the normal map are never
 * written.  Every step below is an IEEE double operation in the order written (the library is built without
 * contraction): add, multiply, divide, sqrt, fmin / fmax and rint only, so results are defined to the bit.
 *
 *   input           per layer l: normals[l], level 0 of a normal map, width x height texels of normal_pixel_type, rows
 *                   normal_pitch_bytes apart; rough0[l], level 0 of the roughness map, the same size, of
 *                   rough_pixel_type, rows rough_pitch_bytes apart -- it may be the surface of the normals -- or
 *                   rough0 == NULL: base_roughness in every texel; levels[l * (levels_count - 1) + (k - 1)], level k
 *                   of the roughness chain, max(1, width >> k) x max(1, height >> k) tightly packed RGBA32F.
 *   decode          RGBA8 (double)((float)(v / 255.0)), RGBA16F half -> double, RGBA32F as stored
 *   normal          x = (double)c with CFHIP_SPEC_AA_SIGNED_NORMALS, else (double)c * 2.0 - 1.0; with
 *                   CFHIP_SPEC_AA_RECONSTRUCT_Z (two-channel normals) the stored blue is ignored and
 *                   z = sqrt(fmax(0.0, 1.0 - (x*x + y*y))); len = sqrt((x*x + y*y) + z*z); len not finite or not > 0:
 *                   the normal is (0, 0, 1), else x / len component by component; qx = (int64)rint(nx * 2^30), ties
 *                   to even, the same for y and z.
 *   roughness       r = the decoded `channel` (or base_roughness); r >= 0 false (a NaN too): r = 0; r > 1: r = 1;
 *                   alpha = r * r with CFHIP_SPEC_AA_PERCEPTUAL (the stored value is perceptual roughness), else r;
 *                   qa = (int64)rint(alpha*alpha * 2^32).
 *   footprint       of texel (x, y) of level k: the level-0 columns [x 2^k, (x + 1) 2^k), but to `width` for the last
 *                   column of the level (x == w_k - 1); the same for rows.  Every level-0 texel belongs to exactly one
 *                   texel of each level, and level k's texel is the union of level k-1's 2x and 2x + 1, plus 2x + 2 at
 *                   an odd end: a 3 x 3 map has a 1 x 1 level 1 of all nine texels.
 *   moments         Sx, Sy, Sz, Sa: the int64 sums of qx, qy, qz, qa over the footprint, N its texels.  A surface has at
 *                   most 2^30 texels, so the sums fit; integer sums are exact in any order.
 *   level texel     int64 -> double rounds to nearest even.  mx = (double)Sx / ((double)N * 2^30), the same for my, mz;
 *                   A2 = (double)Sa / ((double)N * 2^32); L2 = (mx*mx + my*my) + mz*mz.
 *                     L2 < 1.0 false: v = 0
 *                     else L2 > 0 false: v = max_variance                                              (clamped)
 *                     else L = sqrt(L2), t = (1.0 - L2) / (L * (3.0 - L2)), 1 / kappa of the vMF lobe of mean length L,
 *                          v = fmin((double)max_variance, t)                         (clamped iff t < max_variance false)
 *                   a2 = fmin(1.0, A2 + (double)variance_scale * v)   (saturated iff the sum < 1.0 is false)
 *                   stored: (float)sqrt(a2), with PERCEPTUAL (float)sqrt(sqrt(a2))
 *   results_device  layers * (levels_count - 1) records, [l * (levels_count - 1) + (k - 1)], or NULL for none: clamped
 *                   and saturated texels of the level, max_added = the largest (float)((double)variance_scale * v) of
 *                   the level as its bit pattern (an unsigned maximum: the values are not negative), reserved = 0.
 *
 * variance_scale 1 and max_variance 1 are the plain vMF form; 2 and 0.18 give the clamp of Kaplanyan et al.
 * CFHIP_E_INVALID, before anything is enqueued: unknown flags, struct_size != sizeof(cfhip_spec_aa_params), channel > 3,
 * a variance_scale or max_variance that is negative or not finite, base_roughness outside [0, 1], non-zero reserved
 * words, levels_count < 2 or beyond the chain of width x height, layers outside 1 to 65535, sides outside 1 to 32768,
 * more than 2^30 texels in a surface, a pitch below a row, normals[] or normal_pitch_bytes not aligned to a texel of
 * their pixel type (4, 8 or 16 bytes: a normal is one load), rough0[] or rough_pitch_bytes not aligned to a component,
 * levels[] entries not 16-byte aligned, a NULL entry.
 *
 * All layers share every launch, and a launch finishes five levels: a workgroup owns a 32 x 32 tile of its input (the
 * last tile of a row or column takes the remainder, up to 63), reads it once, reduces the moments in LDS, stores the
 * roughness of five levels and leaves the tile's moments (32 bytes) in the context's scratch for the next launch, whose
 * input they are.  ceil((levels_count - 1) / 5) launches per call -- at most 3 -- on the call's stream; level 0 is read
 * once; nothing waits for the host.  stream == NULL means the context's stream and the call synchronises.  Identical
 * calls return identical bytes. */
enum { CFHIP_SPEC_AA_PERCEPTUAL = 1, CFHIP_SPEC_AA_SIGNED_NORMALS = 2, CFHIP_SPEC_AA_RECONSTRUCT_Z = 4 };
typedef struct cfhip_spec_aa_params {
	uint32_t struct_size;
	uint32_t flags;
	uint32_t channel;
	float base_roughness;
	float variance_scale;
	float max_variance;
	uint32_t reserved[2];
} cfhip_spec_aa_params;
typedef struct cfhip_spec_aa_result {
	uint32_t clamped;
	uint32_t saturated;
	uint32_t max_added;
	uint32_t reserved;
} cfhip_spec_aa_result;
int cfhip_spec_aa_array_device(cfhip_ctx* ctx, const void* const* normals, uint32_t layers, int normal_pixel_type,
	uint32_t width, uint32_t height, size_t normal_pitch_bytes, const void* const* rough0, int rough_pixel_type,
	size_t rough_pitch_bytes, void* const* levels, uint32_t levels_count, const cfhip_spec_aa_params* params,
	cfhip_spec_aa_result* results_device, void* stream);

/* Ambient occlusion from height maps, by a horizon scan: the occlusion a height field casts on itself, the third map of
 * an ORM set beside the normals (CFHIP_IMAGE_OP_NORMAL_MAP) and the roughness (above).  For every texel the highest
 * horizon within `radius` texels is found in D directions; the share of the sky above a flat surface that each horizon
 * hides is summed over the directions.  Every step below is an IEEE double operation in the order written (the library
 * is built without contraction): add, subtract, multiply, divide, sqrt and fmin / fmax only, so results are defined to
 * the bit.
 *
 *   input           `layers` source surfaces src[l] of one size width x height (1 to 32768 each, at most 2^30 texels)
 *                   and one pixel type, rows src_pitch_bytes apart, only read.  h(p) is component `channel` (0 to 3),
 *                   decoded as the pass above decodes: RGBA8 (float)(v / 255.0), RGBA16F half -> float, RGBA32F as
 *                   stored.  A non-finite h reads 0.  H(p) = (double)height * (double)h(p): the product of two floats is
 *                   exact.  height is finite, may be negative (an inverted map), and is in texels per stored unit --
 *                   the meaning the normal-map op's height has, so one value gives consistent normals and occlusion.
 *   directions      D = 8, 16 or 32.  The base vectors of the first quadrant:
 *                     D = 8:  (1,0) (1,1)
 *                     D = 16: (1,0) (2,1) (1,1) (1,2)
 *                     D = 32: (1,0) (3,1) (2,1) (3,2) (1,1) (2,3) (1,2) (1,3)
 *                   Direction d = q * D/4 + i is base i turned q times by (x, y) -> (-y, x).  Samples lie on texel
 *                   centres: there is no interpolation.  The weight w_d is half the angle between the two neighbours of
 *                   d, divided by 2 pi, as the nearest double -- but for (1,0) and (3,1) of D = 32 (and their three
 *                   turns), which are one unit in the last place above it: so every set sums to exactly 1.0 in the
 *                   order of the directions, and a flat surface comes out as exactly 1.
 *                   cfhip_height_ao_directions exports the table.
 *   reach           radius R: an integer, 1 to 64, in texels.  R_d is the largest k with k^2 (vx^2 + vy^2) <= R^2,
 *                   decided in integers; it may be 0.  len_d = sqrt((double)(vx^2 + vy^2));
 *                   r(d, k) = 1.0 / ((double)k * len_d); with CFHIP_HAO_FALLOFF
 *                   g(d, k) = r(d, k) * (1.0 - (double)(k^2 (vx^2 + vy^2)) / (double)((R + 1)^2)), else g = r.
 *   horizon         the samples q = p + k v_d, k = 1 ... R_d.  On an axis wrapped by CFHIP_HAO_WRAP_X / _Y the coordinate
 *                   is taken modulo the side (a surface narrower than R is walked more than once); outside an unwrapped
 *                   surface there is no sample.  m_d = the maximum over the samples of (H(q) - H(p)) * g(d, k);
 *                   t_d = fmax(0.0, m_d - (double)bias), and t_d = 0 with no sample.
 *   visibility      cosine-weighted, the default: vis_d = 1.0 / (1.0 + t_d*t_d), which is 1 - sin^2 of the horizon's
 *                   elevation; with CFHIP_HAO_UNIFORM vis_d = 1.0 - t_d / sqrt(1.0 + t_d*t_d).  The surface normal is +z.
 *   value           S = 0.0; for d = 0 ... D - 1 in that order S = S + w_d * vis_d;
 *                   v = fmin(1.0, fmax(0.0, 1.0 - (double)strength * (1.0 - S))).
 *   store           dst[l] is width x height texels of dst_pixel_type, rows dst_pitch_bytes apart.  channel_mask (bits
 *                   R = 1, G = 2, B = 4, A = 8, not 0) names the components that receive v: RGBA8 takes
 *                   (uint8)floor(v * 255 + 0.5), RGBA32F (float)v, RGBA16F (float)v rounded to half, nearest-even.  The
 *                   other components are not written.  dst[l] may equal src[l] when the pixel types are equal, whatever
 *                   the mask: all heights are read before anything is written.
 *   results_device  one record per layer, or NULL for none: occluded (texels with any t_d > 0), darkest (the smallest
 *                   (float)v of the layer as its bit pattern), two reserved zeros.  Identical calls return identical
 *                   bytes.
 *
 * CFHIP_E_INVALID, before anything is enqueued: unknown flags, struct_size != sizeof(cfhip_height_ao_params),
 * channel > 3, directions not 8, 16 or 32, radius outside 1 to 64, a channel_mask of 0 or above 15, a height that is not
 * finite, a strength or bias that is negative or not finite, a non-zero reserved word, layers outside 1 to 65535, sides
 * outside 1 to 32768, more than 2^30 texels in a surface, a pitch below a row, a pointer or pitch not aligned to a
 * component of its pixel type, a NULL entry, dst[l] == src[l] with different pixel types.
 *
 * All layers share both launches: a plane pass (h of every texel as a float, 4 bytes per texel of the context's scratch,
 * grown on demand) and the scan (a workgroup stages a tile of 64 x 16 texels -- 64 x 64 above R = 16 -- and a halo of R
 * in LDS and walks every direction from there).  2 plain launches per call whatever the layers, directions or radius,
 * on the call's stream; nothing waits for the host.  stream == NULL means the context's stream and the call
 * synchronises. */
enum { CFHIP_HAO_WRAP_X = 1, CFHIP_HAO_WRAP_Y = 2, CFHIP_HAO_UNIFORM = 4, CFHIP_HAO_FALLOFF = 8 };
typedef struct cfhip_height_ao_params {
	uint32_t struct_size;
	uint32_t flags;
	uint32_t channel;
	uint32_t directions;
	uint32_t radius;
	uint32_t channel_mask;
	float height;
	float strength;
	float bias;
	uint32_t reserved;
} cfhip_height_ao_params;
typedef struct cfhip_height_ao_result {
	uint32_t occluded;
	uint32_t darkest;
	uint32_t reserved[2];
} cfhip_height_ao_result;
int cfhip_height_ao_array_device(cfhip_ctx* ctx, const void* const* src, uint32_t layers, int src_pixel_type,
	uint32_t width, uint32_t height, size_t src_pitch_bytes, void* const* dst, int dst_pixel_type,
	size_t dst_pitch_bytes, const cfhip_height_ao_params* params, cfhip_height_ao_result* results_device, void* stream);

/* The direction table of the pass above (host only, no context): vx[d], vy[d] and weight[d] for d = 0 ... directions - 1.
 * The library carries the weights as 17-digit literals, within a unit in the last place of half the angle between a
 * direction's neighbours over 2 pi; S = 0.0, S = S + weight[d] in the order of d ends at exactly 1.0.  Any of the
 * three outputs may be NULL.  CFHIP_E_INVALID for a `directions` that is not 8, 16 or 32. */
int cfhip_height_ao_directions(uint32_t directions, int32_t* vx, int32_t* vy, double* weight);

/* Environment maps for image-based lighting: an equirectangular panorama onto the six faces of a cube, the cube's
 * GGX-prefiltered mip chain (level k = the environment convolved with a lobe of roughness r_k), and its projection on
 * nine spherical-harmonic coefficients (the diffuse term).  Every formula below is a sequence of IEEE double operations
 * in the order written (the library is built without contraction), so results are defined to the bit -- but for atan2
 * and asin of the panorama pass and cos, sin and log2 of the table helper, which are the math library's.
 *
 *   faces           CubeFace order +X, -X, +Y, -Y, +Z, -Z; a face is n x n texels (x, y), y downward, tightly packed
 *                   RGBA32F, 16-byte aligned.  s = 2 (x + 0.5) / n - 1, t = 2 (y + 0.5) / n - 1.
 *   d(f, s, t)      +X (1, -t, -s)   -X (-1, -t, s)   +Y (s, 1, t)   -Y (s, -1, -t)   +Z (s, -t, 1)   -Z (-s, -t, -1);
 *                   |d|^2 = (dx^2 + dy^2) + dz^2, n^ = d / sqrt(|d|^2) component by component.
 *   to a face       the major axis of a direction is X if |x| >= |y| and |x| >= |z|, else Y if |y| >= |z|, else Z; a
 *                   negative major component picks the -face.  (s, t) invert the table above, divided by the major
 *                   component's magnitude.
 *   fetch           seamless and bilinear, of a direction from a face set of size n: px = (s + 1) 0.5 n - 0.5,
 *                   x0 = floor(px), fx = px - x0, the same in y.  A tap (i, j) inside [0, n)^2 is that face's texel.  A
 *                   tap outside -- a corner tap too -- is replaced: its centre's (s', t') on the extended face plane
 *                   becomes a direction by the face's formula, the face is selected again, and the nearest texel there
 *                   is taken, floor((s'' + 1) 0.5 n) held to [0, n - 1].  Per channel
 *                   ((c00 (1 - fx) + c10 fx) (1 - fy)) + ((c01 (1 - fx) + c11 fx) fy).
 *   sum64           of v_0 ... v_{m-1}, m a multiple of 64: p_j = the sum of v_i, i = j mod 64, added in increasing i to
 *                   0.0; then p_j += p_{j xor 32}, then xor 16, 8, 4, 2, 1; the result is p_0.
 *
 * cfhip_equirect_to_cube_device: src is one width x height surface (2 <= width, 1 <= height, both <= 32768) of any of
 * the three pixel types, rows src_pitch_bytes apart, read as the alpha passes above read alpha (RGBA8
 * (float)(v / 255.0), RGBA16F half -> float, RGBA32F as stored) with no colour-space change; faces[6] are device
 * pointers, face_size 1 to 8192.  supersample q in {1, 2, 4}: sub-sample (a, b) of texel (x, y) uses
 * s = 2 (x + (a + 0.5) / q) / n - 1 and t likewise; its direction d gives phi = atan2(dx, dz), psi = asin(dy / sqrt(|d|^2)),
 * u = (phi / (2 pi) + 0.5) width - 0.5, v = (0.5 - psi / pi) height - 0.5, and a bilinear fetch in the expression order
 * above with x taps wrapped modulo the width and y taps clamped: the panorama's centre column looks along +Z, its top
 * row along +Y.  The sub-samples are added to 0.0, b outer, a inner, the sum is divided by q^2 and stored as float.  One
 * launch writes the six faces.
 *
 * cfhip_cube_prefilter_device: src_levels is a host table [6][source_levels] (face-major) of device pointers, level l of
 * size max(1, face_size >> l) -- what cfhip_generate_mips_array_device leaves; dst_levels a host table [6][dst_count],
 * level k of size max(1, face_size >> k); no destination may be a source.  tables[k] is host memory: table_samples[k]
 * records of destination level k, a multiple of 64 from 64 to 4096, each a tangent-space light direction (lz >= 0 is also
 * its weight) and a source level of detail, all finite, 0 <= lod <= 14.  table_samples[k] == 0 copies source level k's
 * bits (roughness 0; k < source_levels).  For an output texel with n^ as above: tx = normalise(up x n^) with
 * up = (0, 0, 1), up x n^ = (-ny, nx, 0), where |nz| < 0.999, else up = (1, 0, 0), up x n^ = (0, -nz, ny);
 * ty = n^ x tx; record i has the world direction l = (tx lx + ty ly) + n^ lz per component,
 * l0 = min((int)lod, L - 1), l1 = min(l0 + 1, L - 1), g = lod - (int)lod,
 * c_i = fetch(l0, l) (1 - g) + fetch(l1, l) g, v_i = c_i lz; the texel is (float)(sum64(v) / sum64(lz)) per channel,
 * alpha included.  One launch per destination level for the six faces; the tables travel through the context's staging.
 *
 * cfhip_ggx_sample_table (host only, no context): Hammersley points xi1 = (i + 0.5) / S, xi2 = the radical inverse of i;
 * alpha = roughness^2 (0 < roughness <= 1), cos^2 theta = (1 - xi1) / (1 + (alpha^2 - 1) xi1),
 * h = (sin theta cos phi, sin theta sin phi, cos theta) with phi = 2 pi xi2, l = 2 hz h - (0, 0, 1);
 * pdf = D_GGX(hz, alpha) / 4 = (alpha^2 / (pi ((hz^2 (alpha^2 - 1) + 1)^2))) / 4,
 * lod = clamp(0.5 log2((1 / (S pdf)) / (4 pi / (6 N^2))) + 1, 0, source_levels - 1); a record with lz <= 0 keeps lx, ly
 * and gets lz = 0, lod = 0, so that S stays fixed.  All in double, rounded to float.
 *
 * cfhip_cube_sh9_device: per texel d omega = (4 / n^2) / (r sqrt(r)), r = (1 + s^2) + t^2, and the nine real basis
 * values of n^ in the order 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2 with the constants 0.282095, 0.488603 (y, z, x),
 * 1.092548 (xy, yz, xz), 0.315392 (3z^2 - 1) and 0.546274 (x^2 - y^2) -- 1 / (2 sqrt(pi)), sqrt(3 / (4 pi)),
 * sqrt(15 / (4 pi)), sqrt(5 / (16 pi)), sqrt(15 / (16 pi)), used at full double precision (csrc/envmap.h).  A row's
 * partials are sum64 over c (Y d omega) and over d omega, the row padded with zeros to a multiple of 64; the rows are
 * added in (face, y) order to 0.0; each of the 36 sums is multiplied by (4 pi) / (the sum of d omega).  The record is
 * those 36 doubles, coefficient-major, then the sum of d omega.  Two launches; identical calls give identical bytes.
 *
 * Every argument is checked before anything is enqueued; stream == NULL means the context's stream and the call
 * synchronises.  The scratch is the context's. */
typedef struct cfhip_ggx_sample {
	float lx, ly, lz;
	float lod;
} cfhip_ggx_sample;
typedef struct cfhip_sh9_result {
	double coeff[9][4];
	double solid_angle;
} cfhip_sh9_result;
int cfhip_equirect_to_cube_device(cfhip_ctx* ctx, const void* src, int src_pixel_type, uint32_t width, uint32_t height,
	size_t src_pitch_bytes, void* const* faces, uint32_t face_size, uint32_t supersample, void* stream);
int cfhip_ggx_sample_table(float roughness, uint32_t samples, uint32_t face_size, uint32_t source_levels,
	cfhip_ggx_sample* out);
int cfhip_cube_prefilter_device(cfhip_ctx* ctx, const void* const* src_levels, uint32_t face_size, uint32_t source_levels,
	void* const* dst_levels, uint32_t dst_count, const cfhip_ggx_sample* const* tables, const uint32_t* table_samples,
	void* stream);
int cfhip_cube_sh9_device(cfhip_ctx* ctx, const void* const* faces, uint32_t face_size, cfhip_sh9_result* result_device,
	void* stream);

/* The rest of what a split-sum shader with GGX, sheen and diffuse terms reads: sample tables of two more lobes for the
 * prefilter above, the BRDF lookup table (the split sum's second factor) and a rendered irradiance cube.  The vocabulary
 * (faces, n^, sum64, IEEE double in the written order) is that of the comment above; pow of the Charlie terms and cos,
 * sin, log2 of the table helpers are the math library's.
 *
 * cfhip_lobe_sample_table (host only, no context): `samples` records for one destination level of
 * cfhip_cube_prefilter_device, from the Hammersley points of cfhip_ggx_sample_table (xi1 = (i + 0.5) / S, xi2 = the
 * radical inverse of i, phi = 2 pi xi2), S a multiple of 64 from 64 to 4096, all in double, rounded to float.
 *   kind 0, GGX      exactly cfhip_ggx_sample_table(roughness, ...).
 *   kind 1, Charlie  alpha = roughness^2 (0 < roughness <= 1); sin theta = pow(xi1, alpha / (2 alpha + 1)),
 *                    cos theta = sqrt(1 - sin^2 theta); h = (sin theta cos phi, sin theta sin phi, cos theta),
 *                    l = 2 hz h - (0, 0, 1) as (2 hz) hx, (2 hz) hy, (2 hz) hz - 1;
 *                    pdf = D / 4, D = ((2 + 1 / alpha) pow(sin theta, 1 / alpha)) / (2 pi);
 *                    lod = clamp(0.5 log2((1 / (S pdf)) / (4 pi / (6 N^2))) + 1, 0, source_levels - 1) -- a pdf of 0
 *                    gives the last level; a record with lz <= 0 keeps lx, ly and gets lz = 0, lod = 0.
 *   kind 2, Lambert  uniform over the hemisphere, because the prefilter weighs every record by lz: the level is then
 *                    the integral of L cos over the integral of cos, the irradiance over pi.  roughness is not read;
 *                    lz = 1 - xi1, sin theta = sqrt(1 - lz^2), l = (sin theta cos phi, sin theta sin phi, lz);
 *                    pdf = 1 / (2 pi), so the lod -- the same formula -- is one value for the table.
 * CFHIP_E_INVALID, with nothing written, for any other kind, a NULL out, samples, face_size or source_levels outside
 * what cfhip_ggx_sample_table takes, and for kinds 0 and 1 a roughness outside (0, 1].
 *
 * cfhip_hammersley_table (host only, no context): record i is (float)cos phi, (float)sin phi, (float)xi1, 0 of the same
 * points -- what cfhip_brdf_lut_device reads.  CFHIP_E_INVALID for a NULL out or such a `samples`.
 *
 * cfhip_brdf_lut_device: dst is width x height (1 to 1024 each) tightly packed RGBA32F on the device, 16-byte aligned;
 * table is host memory, `samples` records (a multiple of 64 from 64 to 4096), each finite with 0 < xi1 < 1; it travels
 * through the context's staging.  sheen is 0 or 1.  Texel (x, y): NoV = (x + 0.5) / width, r = (y + 0.5) / height,
 * alpha = r r, a2 = alpha alpha, v = (vx, 0, vz) = (sqrt(1 - NoV NoV), 0, NoV).  With c = (double)cos_phi and
 * xi = (double)xi1 of record i:
 *   GGX      c2 = (1 - xi) / (1 + (a2 - 1) xi), hz = sqrt(c2), st = sqrt(1 - c2), hx = st c, VoH = (vx hx) + (vz hz),
 *            NoL = (2 VoH) hz - vz.  Where NoL > 0 and VoH > 0:
 *            vis = 0.5 / (NoL sqrt((NoV NoV) (1 - a2) + a2) + NoV sqrt((NoL NoL) (1 - a2) + a2)),
 *            t = ((vis VoH) NoL) / hz, m = 1 - VoH, fc = ((m m) (m m)) m, A_i = (1 - fc) t, B_i = fc t; else both 0.
 *            R = (float)((4 sum64(A)) / S), G = (float)((4 sum64(B)) / S): the scale and the bias of F0 under the
 *            height-correlated Smith term and Schlick's Fresnel.
 *   Charlie  with sheen: hz = 1 - xi (uniform half vectors), st = sqrt(1 - hz hz), hx, VoH and NoL as above.  Under the
 *            same condition vn = 1 / (4 ((NoL + NoV) - NoL NoV)), d = ((2 + 1 / alpha) pow(st, 1 / alpha)) / (2 pi),
 *            C_i = ((vn d) NoL) VoH; else 0.  B = (float)(((8 pi) sum64(C)) / S): the sheen lobe's directional albedo.
 *            Without sheen B = 0.
 * Alpha is 1.  One launch, a wavefront per texel; identical calls give identical bytes.
 *
 * cfhip_cube_irradiance_device: sh9_result_device is the record cfhip_cube_sh9_device left on the device (8-byte
 * aligned, only read; no host round trip); faces[6] as above, face_size 1 to 8192, none equal to the record.  For a
 * texel's n^ = (x, y, z) the nine basis values Y_b of cfhip_cube_sh9_device's order and constants, and the cosine
 * lobe's band factors k_b = pi for b = 0, (2 pi) / 3 for b = 1 ... 3, pi / 4 for b = 4 ... 8: per channel E = 0.0,
 * E = E + (k_b Y_b) coeff[b][c] for b = 0 ... 8 in that order; with over_pi (0 or 1) set E = E / pi; the texel is
 * (float)E, alpha included.  One launch writes the six faces.
 *
 * Every argument is checked before anything is enqueued; stream == NULL means the context's stream and the call
 * synchronises. */
enum { CFHIP_LOBE_GGX = 0, CFHIP_LOBE_CHARLIE = 1, CFHIP_LOBE_LAMBERT = 2 };
typedef struct cfhip_hammersley_sample {
	float cos_phi, sin_phi;
	float xi1;
	float reserved;
} cfhip_hammersley_sample;
int cfhip_lobe_sample_table(int kind, float roughness, uint32_t samples, uint32_t face_size, uint32_t source_levels,
	cfhip_ggx_sample* out);
int cfhip_hammersley_table(uint32_t samples, cfhip_hammersley_sample* out);
int cfhip_brdf_lut_device(cfhip_ctx* ctx, void* dst, uint32_t width, uint32_t height, const cfhip_hammersley_sample* table,
	uint32_t samples, uint32_t sheen, void* stream);
int cfhip_cube_irradiance_device(cfhip_ctx* ctx, const cfhip_sh9_result* sh9_result_device, void* const* faces,
	uint32_t face_size, uint32_t over_pi, void* stream);

/* One Image::resize on the GPU (lib/src/Image.cpp:1324-1511) -- what Texture::generateMipmaps calls
 * per level, and per custom mip image (Texture.cpp:1499-1503, any source size): src (any of the
 * three pixel types) -> dst, dst_width x dst_height tightly packed RGBA32F, in linear space as
 * above; equal sizes copy the texels (Image.cpp:1330-1334).  Same filters, same stream rule. */
int cfhip_resize_device(cfhip_ctx* ctx, const void* src, int src_pixel_type, uint32_t src_width,
	uint32_t src_height, size_t src_pitch_bytes, int color_space, int filter, void* dst,
	uint32_t dst_width, uint32_t dst_height, void* stream);

/* The same for a 3-D texture (Texture::generateMipmaps, Dim3D branch, lib/src/Texture.cpp:1345-1440):
 * level k = every slice of level k-1 resized to max(1, w >> k) x max(1, h >> k) by Image::resize, then
 * generateMips3d (Texture.cpp:103-227) along the depth to max(1, depth >> k) slices -- Box counts
 * the slices inside the footprint, every other filter weights them with a tent.  src: `depth`
 * slices, src_slice_pitch_bytes apart; dst_levels[k - 1]: level k as tightly packed RGBA32F
 * slices (w_k * h_k * 16 bytes each, depth_k of them). */
int cfhip_generate_mips3d_device(cfhip_ctx* ctx, const void* src, int src_pixel_type,
	uint32_t width, uint32_t height, uint32_t depth, size_t src_pitch_bytes,
	size_t src_slice_pitch_bytes, int color_space, int filter, void* const* dst_levels,
	uint32_t levels, void* stream);

/* Block-row sharding of one surface across `world` ranks:
 * rank r owns block rows [*row_begin, *row_end).  Pure function, no communication. */
int cfhip_shard_rows(uint32_t block_rows, int rank, int world, uint32_t* row_begin,
	uint32_t* row_end);

/* ---- Decoding: the payload of every block format back to texels, on the GPU ----
 *
 * Output is bit-identical to the project's CPU reference decoders, which are pinned to Pillow (BC1-5, BC7)
 * and Mesa 23.2.1 (ETC2, EAC, BC7, BC6H, ASTC) through committed fixtures.  Every legal block decodes, also
 * encodings this library never emits (all ASTC block modes, grids and partition seeds).
 * Texels are row-major, top-down; partial edge blocks write only the texels inside width x height.
 * Colour space: the stored values are returned.  No sRGB transfer is applied and ASTC's sRGB decode mode is
 * not modelled (an sRGB payload decodes to its sRGB-encoded values).
 *
 * Decoded layouts (cfhip_decoded_layout):
 *   BC1, BC1A, BC2, BC3, BC7, ETC1, ETC2 x3, ASTC UNorm   RGBA8              4 bytes per texel
 *   BC4 UNorm / SNorm                                      R8 / R8 signed     1
 *   BC5 UNorm / SNorm                                      RG8 / RG8 signed   2
 *   EAC R11 / RG11 UNorm / SNorm                           R16 / RG16 holding the 11-bit value,
 *                                                          0..2047 or -1023..1023          2 / 4
 *   BC6H UFloat / Float, ASTC UFloat                       RGBA16F bit patterns (BC6H alpha 1.0)   8
 * BC1 three-colour blocks decode index 3 to transparent black.  ASTC: an illegal block decodes to magenta
 * (LDR) or to 0xFFFF halves (HDR); under the LDR profile a partition with HDR endpoints decodes to magenta.
 *
 * Error blocks: the blocks whose reference decoder reports an error -- BC6H reserved modes, ASTC illegal
 * blocks and (LDR profile) ASTC blocks with a texel in a partition with HDR endpoints.  0 for the other
 * formats.
 *
 * Stream and error rules are those of the encode entry points: stream == NULL means the context's stream and
 * the call synchronises; every argument is checked before anything is enqueued. */
enum cfhip_layout {
	CFHIP_LAYOUT_RGBA8 = 0,
	CFHIP_LAYOUT_R8 = 1,
	CFHIP_LAYOUT_R8_SNORM = 2,
	CFHIP_LAYOUT_RG8 = 3,
	CFHIP_LAYOUT_RG8_SNORM = 4,
	CFHIP_LAYOUT_R16 = 5,           /* EAC R11 unsigned, 0..2047 */
	CFHIP_LAYOUT_R16_SNORM = 6,     /* EAC R11 signed, -1023..1023 */
	CFHIP_LAYOUT_RG16 = 7,
	CFHIP_LAYOUT_RG16_SNORM = 8,
	CFHIP_LAYOUT_RGBA16F = 9,
	CFHIP_LAYOUT_RGBA32F = 10       /* what cfhip_std_unpack writes; no block (format, type) pair decodes to it */
};

/* Decoded texel layout of a block (format, type) pair; CFHIP_E_UNSUPPORTED for the standard formats and for
 * the pairs cfhip_query rejects.  Pure, needs no device. */
int cfhip_decoded_layout(int format, int type, int* layout, int* texel_bytes);

/* Host buffers: blocks (blocks_bytes >= the payload size of width x height) -> out, width * height texels
 * tightly packed (out_capacity >= width * height * texel_bytes, else CFHIP_E_CAPACITY).  error_blocks
 * (optional) receives the number of error blocks.  Blocking. */
int cfhip_decode(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes,
	uint32_t width, uint32_t height, void* out, size_t out_capacity, uint64_t* error_blocks);

/* Device buffers: blocks and out are device pointers on ctx's GPU, out rows out_pitch_bytes apart
 * (>= width * texel_bytes).  error_blocks_device: one uint64 on the device, zeroed by the call on the stream
 * and then receiving the count; NULL: not counted. */
int cfhip_decode_device(cfhip_ctx* ctx, int format, int type, const void* blocks,
	uint32_t width, uint32_t height, void* out, size_t out_pitch_bytes,
	uint64_t* error_blocks_device, void* stream);

/* ---- Batched decode: every surface of a texture (mip chain, cube faces, array layers) in ONE launch, to the
 * native layout or to pixels an encoder, cfhip_image_ops_device or cfhip_generate_mips*_device can read ----
 *
 * Formats 29..56, the pairs cfhip_query accepts; standard formats and PVRTC are CFHIP_E_UNSUPPORTED (they keep
 * their own per-surface entries).  out_pixel is CFHIP_DECODE_NATIVE or a cfhip_pixel_type; the values are the
 * ones cfhip_compare documents, absent channels 0, 0, 1, every quotient the correctly rounded single:
 *
 *   native layout        RGBA8                 RGBA16F            RGBA32F
 *   RGBA8, R8, RG8       the bytes, expanded   unsupported        (float)(v / 255.0)
 *   R8 / RG8 SNorm       unsupported           unsupported        (float)max(v / 127.0, -1)
 *   R16 / RG16 (EAC)     unsupported           unsupported        (float)(v / 2047.0), signed (float)max(v / 1023.0, -1)
 *   RGBA16F              unsupported           the bit patterns   the half widened exactly
 *
 * An unsupported cell is CFHIP_E_UNSUPPORTED; cfhip_decode_out_supported answers the table (1 / 0) without a
 * device.  Each surface decodes exactly as cfhip_decode decodes it; error blocks are counted per surface.
 * One launch per call: a surface table travels through the context's staging and every workgroup finds its
 * surface by a wave-uniform binary search.  n == 0 is CFHIP_OK and does nothing.
 * Stream and error rules are those of cfhip_decode*: every argument of every surface is checked before anything
 * is enqueued (and before ctx is looked at: a NULL ctx is reported last); stream == NULL means the context's
 * stream and the call synchronises. */
typedef struct cfhip_decode_surface {
	const void* blocks;      /* payload of this surface */
	size_t blocks_bytes;     /* host form: >= its payload size; device form: ignored */
	uint32_t width, height;
	void* out;               /* texels, rows out_pitch_bytes apart */
	size_t out_pitch_bytes;  /* >= width * bytes per output texel */
	size_t out_capacity;     /* host form: >= (height - 1) * pitch + width * texel bytes, else CFHIP_E_CAPACITY */
} cfhip_decode_surface;
#define CFHIP_DECODE_NATIVE (-1)   /* the layout cfhip_decoded_layout names */

/* Host buffers.  Surfaces whose blocks are consecutive in host memory (a loaded file) upload as one copy; tightly
 * pitched outputs that are consecutive in host memory come back as one copy.  error_blocks: n counts, or NULL.
 * Blocking. */
int cfhip_decode_batch(cfhip_ctx* ctx, int format, int type, int out_pixel,
	const cfhip_decode_surface* surfaces, size_t n_surfaces, uint64_t* error_blocks);

/* Device buffers: `surfaces` is a host array of device pointers.  16-byte aligned outputs and pitches and
 * block-aligned payloads take the vector paths, per surface; anything else is legal.  error_blocks_device: n
 * uint64 on the device (8-byte aligned), zeroed by the call on the stream, or NULL. */
int cfhip_decode_batch_device(cfhip_ctx* ctx, int format, int type, int out_pixel,
	const cfhip_decode_surface* surfaces, size_t n_surfaces, uint64_t* error_blocks_device, void* stream);

/* 1 where (format, type) decodes to out_pixel, else 0.  Pure, needs no device. */
int cfhip_decode_out_supported(int format, int type, int out_pixel);

/* Decode and compare in one pass, without writing texels: sse[c] = the exact sum over the width x height
 * texels of (decoded - reference)^2 of channel c.  ref_rgba8: RGBA8 rows ref_pitch_bytes apart
 * (>= width * 4).  Layouts RGBA8, and R8 / RG8 (BC4 / BC5 UNorm), which compare R (and G) and report 0 for
 * the absent channels; every other pair is CFHIP_E_UNSUPPORTED. */
int cfhip_decode_sse(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes,
	uint32_t width, uint32_t height, const void* ref_rgba8, size_t ref_pitch_bytes, uint64_t sse[4]);

/* The same on device buffers: sse_device = four uint64 on the device, zeroed by the call on the stream.  It must
 * be 8-byte aligned (the kernels add to it with 64-bit atomics); otherwise CFHIP_E_INVALID, nothing enqueued. */
int cfhip_decode_sse_device(cfhip_ctx* ctx, int format, int type, const void* blocks,
	uint32_t width, uint32_t height, const void* ref_rgba8, size_t ref_pitch_bytes,
	uint64_t* sse_device, void* stream);

/* ---- per-image pixel operations (Image.cpp:1513-1882): the steps the cuttlefish tool runs between loading an
 * image and Texture::setImage (tool/main.cpp:147-277), except the resizes ---- */

/* cuttlefish::Image::Channel (Image.h:104-111) */
enum cfhip_channel {
	CFHIP_CHANNEL_RED = 0,
	CFHIP_CHANNEL_GREEN = 1,
	CFHIP_CHANNEL_BLUE = 2,
	CFHIP_CHANNEL_ALPHA = 3,
	CFHIP_CHANNEL_NONE = 4     /* 0 for red, green and blue, 1 for alpha */
};

/* cuttlefish::Image::RotateAngle (Image.h:91-99) */
enum cfhip_rotate {
	CFHIP_ROTATE_CW90 = 0,
	CFHIP_ROTATE_CW180 = 1,
	CFHIP_ROTATE_CW270 = 2,
	CFHIP_ROTATE_CCW90 = 3,
	CFHIP_ROTATE_CCW180 = 4,
	CFHIP_ROTATE_CCW270 = 5
};

/* cuttlefish::Image::NormalOptions (Image.h:116-122), a bit mask */
enum cfhip_normal_options {
	CFHIP_NORMAL_DEFAULT = 0,
	CFHIP_NORMAL_KEEP_SIGN = 1,
	CFHIP_NORMAL_WRAP_X = 2,
	CFHIP_NORMAL_WRAP_Y = 4
};

/* The ops of one cfhip_image_ops_device call; they run in this order (the tool's), whatever the order of the bits */
enum cfhip_image_op {
	CFHIP_IMAGE_OP_COLOR_SPACE = 1 << 0,   /* Image::changeColorSpace(dst_color_space) */
	CFHIP_IMAGE_OP_ROTATE = 1 << 1,        /* Image::rotate(rotate) */
	CFHIP_IMAGE_OP_GRAYSCALE = 1 << 2,     /* Image::grayscale() */
	CFHIP_IMAGE_OP_NORMAL_MAP = 1 << 3,    /* Image::createNormalMap(normal_options, normal_height): RGBF from here */
	CFHIP_IMAGE_OP_FLIP_X = 1 << 4,        /* Image::flipHorizontal() */
	CFHIP_IMAGE_OP_FLIP_Y = 1 << 5,        /* Image::flipVertical() */
	CFHIP_IMAGE_OP_SWIZZLE = 1 << 6,       /* Image::swizzle(swizzle[0..3]) */
	CFHIP_IMAGE_OP_PREMULTIPLY = 1 << 7    /* Image::preMultiplyAlpha() */
};

typedef struct cfhip_image_ops {
	uint32_t ops;              /* cfhip_image_op bits */
	int32_t src_color_space;   /* the image's colour space (cfhip_color_space) */
	int32_t dst_color_space;   /* CFHIP_IMAGE_OP_COLOR_SPACE: the space it changes to; later ops use it */
	int32_t rotate;            /* cfhip_rotate, read under CFHIP_IMAGE_OP_ROTATE */
	uint32_t normal_options;   /* cfhip_normal_options bits */
	uint32_t rgbf;             /* 1: the image is RGBF (a normal map): alpha reads 1, a swizzled alpha is dropped,
	                            * premultiplication does nothing */
	double normal_height;
	int32_t swizzle[4];        /* cfhip_channel of the red, green, blue and alpha outputs */
} cfhip_image_ops;

/* One fused pass of the ops above on device buffers.  src: w x h texels of src_pixel_type, rows
 * src_pitch_bytes apart, read as the reference's RGBAF image (RGBA8 as v/255).  dst: the result as RGBA32F,
 * rows dst_pitch_bytes apart, h x w texels under a 90 or 270 degree rotation and w x h otherwise.  Every op
 * rounds to float where the reference stores, so one call equals the same ops one call each, bit for bit.
 * src and dst must not overlap.  stream NULL = the context's stream, and the call then synchronises; on a
 * caller's stream it returns once the launch is queued. */
int cfhip_image_ops_device(cfhip_ctx* ctx, const void* src, int src_pixel_type, uint32_t w, uint32_t h,
	size_t src_pitch_bytes, const cfhip_image_ops* ops, void* dst, size_t dst_pitch_bytes, void* stream);

/* ---- Quality metrics: an encoded payload against its reference, on the GPU ----
 *
 * The payload is decoded as cfhip_decode decodes it and every texel normalised to double:
 *   RGBA8 / R8 / RG8 v/255; R8 / RG8 signed max(v/127, -1); EAC R16 / RG16 v/2047, signed max(v/1023, -1);
 *   RGBA16F half -> float (BC6H alpha 1.0).
 * The reference is read as stored, without clamp or sRGB transfer: RGBA8 v/255, RGBA16F, RGBA32F.
 * Channels compared: those of the decoded layout (R, RG or RGBA) AND the caller's mask.  For each:
 *   sse[c]      = sum of (dec - ref)^2 over the width x height texels, in FP64
 *   log_sse[c]  = sum of (log2(max(dec, 2^-24)) - log2(max(ref, 2^-24)))^2, RGBA16F layouts only (NaN otherwise)
 *   ref_max[c]  = the maximum of the reference
 *   ssim[c]     = with CFHIP_COMPARE_SSIM, LDR layouts: mean SSIM over the window centres whose 11 x 11 window
 *                 lies inside the surface (Gaussian, sigma 1.5; C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = 1 for UNorm
 *                 and 2 for SNorm layouts).  NaN when not computed, for HDR layouts and when a side is below 11.
 * Channels not compared report 0 (ssim NaN).  error_blocks counts as cfhip_decode counts.  block_errors
 * (optional): one float per block of the payload's block grid, row-major, the block's SSE summed over the
 * compared channels and its texels inside the surface; block_errors_capacity counts floats (>= blocks, else
 * CFHIP_E_CAPACITY).  Partial sums are reduced in a fixed order: identical calls return identical bits. */
typedef struct cfhip_compare_result {
	uint64_t texels, error_blocks;
	uint32_t channels;        /* bit c: channel c compared */
	uint32_t ssim_windows;    /* valid window centres; 0 when SSIM was not computed */
	double sse[4], log_sse[4], ssim[4], ref_max[4];
} cfhip_compare_result;

#define CFHIP_COMPARE_SSIM 1u

/* Host buffers: blocks (blocks_bytes >= the payload size), ref: width x height texels of ref_pixel_type
 * (cfhip_pixel_type), rows ref_pitch_bytes apart.  mask_rgba NULL = every channel.  Blocking.  Standard formats
 * and the pairs cfhip_query rejects are CFHIP_E_UNSUPPORTED. */
int cfhip_compare(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes,
	uint32_t width, uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch_bytes,
	const uint8_t mask_rgba[4], unsigned flags, cfhip_compare_result* result,
	float* block_errors, size_t block_errors_capacity);

/* Device buffers on ctx's GPU: blocks, ref (pointer and pitch aligned to the texel size), result_device and
 * block_errors_device (optional).  mask_rgba is host memory.  stream NULL = the context's stream, and the call
 * then synchronises; on a caller's stream it returns once the work is queued. */
int cfhip_compare_device(cfhip_ctx* ctx, int format, int type, const void* blocks,
	uint32_t width, uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch_bytes,
	const uint8_t mask_rgba[4], unsigned flags, cfhip_compare_result* result_device,
	float* block_errors_device, size_t block_errors_capacity, void* stream);

/* ---- Batched compare: every surface of a texture (mip chain, cube faces, array layers) measured in ONE call ----
 *
 * Each surface is measured exactly as cfhip_compare measures it: the same formats (29..56, the pairs cfhip_query
 * accepts; standard formats and PVRTC are CFHIP_E_UNSUPPORTED and keep their own entries), the same errors and
 * alignment rules, and results[i] holds the very bits cfhip_compare / cfhip_compare_device return for surface i
 * alone.  All surfaces share format, type, ref_pixel_type, mask and flags.
 * The launch count does not depend on n: one Pass A launch over the workgroups of every surface and one final
 * launch with a workgroup per surface; with CFHIP_COMPARE_SSIM (and a surface of at least 11 x 11 texels) one
 * batched decode into scratch and one SSIM launch over the tiles of every surface in between.  A surface table
 * travels through the context's staging and every workgroup finds its surface by a wave-uniform binary search.
 * Surfaces below 11 texels a side report SSIM NaN and 0 windows.  The device scratch (decoded surfaces, partial
 * sums) grows with the sum over the surfaces; it is not capped, so a caller short of memory splits the call.
 * n == 0 is CFHIP_OK and does nothing.  Every argument of every surface is checked before anything is enqueued
 * (and before ctx is looked at: a NULL ctx is reported last). */
typedef struct cfhip_compare_surface {
	const void* blocks;            /* payload of this surface */
	size_t blocks_bytes;           /* host form: >= its payload size; device form: ignored */
	uint32_t width, height;
	const void* ref;               /* width x height texels of ref_pixel_type */
	size_t ref_pitch_bytes;        /* >= width * bytes per reference texel */
	float* block_errors;           /* the surface's error map, or NULL: no map for this surface */
	size_t block_errors_capacity;  /* floats; >= blocks of the surface where block_errors is given, else CFHIP_E_CAPACITY */
} cfhip_compare_surface;

/* Host buffers.  Payloads that are consecutive in host memory (a loaded file) upload as one copy, and so do tightly
 * pitched references that are; the n results come back as one copy, the maps one copy each.  Blocking. */
int cfhip_compare_batch(cfhip_ctx* ctx, int format, int type, const cfhip_compare_surface* surfaces,
	size_t n_surfaces, int ref_pixel_type, const uint8_t mask_rgba[4], unsigned flags,
	cfhip_compare_result* results);

/* Device buffers: `surfaces` is a host array of device pointers (references and their pitches aligned to the texel
 * size, maps to 4 bytes); results_device: n cfhip_compare_result on the device, 8-byte aligned.  mask_rgba is host
 * memory.  stream NULL = the context's stream, and the call then synchronises; on a caller's stream it returns
 * once the work is queued. */
int cfhip_compare_batch_device(cfhip_ctx* ctx, int format, int type, const cfhip_compare_surface* surfaces,
	size_t n_surfaces, int ref_pixel_type, const uint8_t mask_rgba[4], unsigned flags,
	cfhip_compare_result* results_device, void* stream);

/* ---- Rate-distortion optimisation of BC1-5 / BC7 payloads ----
 *
 * A post-pass over an encoded payload: byte ranges of some blocks are overwritten by the same byte range of one of
 * the 16 blocks before them in the same segment (64 blocks) of their block row, so that a deflate-class compressor
 * finds matches.  Per block, candidate 0 is the block as encoded and every other candidate one splice of the
 * format's table taken from one distance d = 1..16; the pass keeps the first minimum of
 *   J = 16 SSE + round(16 lambda) R
 * where SSE is the integer squared error of the decoded candidate against the source as RGBA8 (floats quantised as
 * the encoders quantise them: round(clamp(f) * 255), NaN 0) over the channels the format stores AND mask_rgba
 * (BC1_RGB stores no alpha) and the texels inside the surface, and R its model rate in bits: 8 BS for the block as
 * encoded, 8 (BS - n) + 12 + 2 floor(log2(d BS)) for a splice of n bytes (BS: bytes of a block).  Only candidates
 * with SSE <= SSE(candidate 0) + max_sse_increase take part (0xFFFFFFFF: no cap); a candidate the decoder counts
 * as an error block (BC7's reserved mode) never does.  Blocks are taken left to right and copy from FINAL blocks.
 * Supported: BC1_RGB, BC1_RGBA, BC2, BC3, BC4, BC5 and BC7, type UNorm; every other pair is CFHIP_E_UNSUPPORTED.
 * All surfaces of a call share format, type, parameters and mask, and one launch.  The statistics are integer
 * sums: identical calls return identical bits.  n == 0 is CFHIP_OK and does nothing.  Every argument of every
 * surface is checked before anything is enqueued (and before ctx is looked at: a NULL ctx is reported last). */
typedef struct cfhip_rdo_params {
	float lambda;               /* 0 < lambda <= 1024, else CFHIP_E_INVALID */
	uint32_t max_sse_increase;  /* per block; 0xFFFFFFFF = no cap */
	uint32_t reserved[2];       /* must be 0 */
} cfhip_rdo_params;

typedef struct cfhip_rdo_surface {
	const void* blocks;         /* payload of this surface as encoded */
	size_t blocks_bytes;        /* host form: >= its payload size; device form: ignored */
	void* out;                  /* the optimised payload; may equal blocks (in place), must not overlap it otherwise */
	size_t out_capacity;        /* >= the payload size, else CFHIP_E_CAPACITY */
	uint32_t width, height;
	const void* pixels;         /* the source the payload was encoded from: width x height texels */
	int pixel_type;             /* cfhip_pixel_type */
	size_t row_pitch_bytes;     /* >= width * bytes per texel */
} cfhip_rdo_surface;

typedef struct cfhip_rdo_stats {
	uint64_t blocks, blocks_changed;  /* blocks of the surface; those whose bytes differ from the input */
	uint64_t sse_before, sse_after;   /* summed over the blocks, as defined above */
	uint64_t bits_before, bits_after; /* model rate R summed over the blocks */
} cfhip_rdo_stats;

/* 1 for the (format, type) pairs of the table above, else 0.  Pure, needs no device. */
int cfhip_rdo_supported(int format, int type);

/* Host buffers; stats: n_surfaces entries.  Blocking. */
int cfhip_rdo(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n_surfaces,
	const cfhip_rdo_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats);

/* Device buffers: `surfaces` is a host array of device pointers (pixels and their pitch aligned to the texel size);
 * stats_device: n_surfaces cfhip_rdo_stats on the device, 8-byte aligned, overwritten.  params and mask_rgba are
 * host memory.  stream NULL = the context's stream, and the call then synchronises; on a caller's stream it
 * returns once the work is queued. */
int cfhip_rdo_device(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n_surfaces,
	const cfhip_rdo_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats_device, void* stream);

/* The pass with options.  flags == 0 returns exactly what cfhip_rdo / cfhip_rdo_device return.
 *
 * CFHIP_RDO_ROW_ABOVE: a block may also copy from the block row above (2-D lookback).  A surface is cut into tiles
 * of 64 blocks x 8 block rows, counted from its top-left corner; tiles are independent, and inside a tile rows are
 * taken top to bottom, blocks left to right.  A block at position i of its segment, not in the first row of its tile,
 * has 8 more sources: the FINAL blocks at positions i + dx, dx = -4..3, of the row above in the same tile (those
 * that exist), each with every splice of the format's table.  These candidates follow the 16 S of the plain pass, in
 * the order (dx, splice), and cost R = 8 (BS - n) + 12 + 2 floor(log2((bx - dx) BS)) bits, bx the blocks of a row of
 * the surface: the distance of the match in the payload.  Everything else is the plain pass: J, the first minimum,
 * the cap, the error-block rule, the mask, the statistics.  A surface whose row above lies outside the compressor's
 * window, (bx + 4) BS > window_bytes, gets the plain pass's result.  Surfaces with and without share the one launch. */
#define CFHIP_RDO_ROW_ABOVE 1u

typedef struct cfhip_rdo_ex_params {
	uint32_t struct_size;       /* sizeof(cfhip_rdo_ex_params), else CFHIP_E_INVALID */
	float lambda;               /* as cfhip_rdo_params */
	uint32_t max_sse_increase;  /* as cfhip_rdo_params */
	uint32_t flags;             /* CFHIP_RDO_*; unknown bits are CFHIP_E_INVALID */
	uint32_t window_bytes;      /* the compressor's window: 0 = 32768 (deflate), else 64 .. 2^30 */
	uint32_t reserved[3];       /* must be 0 */
} cfhip_rdo_ex_params;

/* cfhip_rdo with cfhip_rdo_ex_params: same buffers, same checks, the params' fields checked in their order. */
int cfhip_rdo_ex(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n_surfaces,
	const cfhip_rdo_ex_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats);

/* cfhip_rdo_device with cfhip_rdo_ex_params. */
int cfhip_rdo_ex_device(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n_surfaces,
	const cfhip_rdo_ex_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats_device, void* stream);

/* ---- Deflate-size estimate of payloads, and the rate-distortion pass to a target ratio ----
 *
 * How many bytes a byte stream takes inside a zip / PNG-class package, computed on the device for payloads of any
 * format.  The stream (the spans of a call, concatenated; fewer than 2^31 bytes) is parsed the way a deflate encoder
 * parses it -- hash candidates on 4-byte keys (the 4 nearest within 32768 bytes), matches of 4..258 bytes that end at
 * 4096-byte chunk boundaries, one-step lazy evaluation -- and priced, per block of 65536 input bytes, with the
 * zeroth-order entropy of deflate's literal/length and distance alphabets plus their extra bits.  There is no term for
 * the code-table headers, so streams that compress to a few hundred bytes are underestimated.  The definition, down
 * to the fixed-point logarithm, is tests/lzsize_ref.py; every result is an integer sum, so identical calls return
 * identical bits.  Scratch belongs to the context: about 21 bytes per byte of a slice (cfhip_lz_slice_bytes). */
typedef struct cfhip_lz_span {
	const void* bytes;
	size_t n;
} cfhip_lz_span;

typedef struct cfhip_lz_stats {
	uint64_t bytes_in;          /* bytes of the stream */
	uint64_t bits_q16;          /* the estimate in 1/65536 bit */
	uint64_t est_bytes;         /* ceil(bits_q16 / (8 * 65536)) */
	uint64_t literals, matches; /* tokens of the parse */
	uint64_t matched_bytes;     /* bytes covered by matches */
} cfhip_lz_stats;

/* Host spans.  A span of 0 bytes is skipped (its pointer may be NULL); a stream of 0 bytes is CFHIP_OK with all-zero
 * stats and needs no context.  2^31 bytes or more: CFHIP_E_CAPACITY.  Every argument is checked before anything is
 * enqueued (a NULL ctx is reported last).  Blocking. */
int cfhip_lz_size(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, cfhip_lz_stats* out);

/* Device spans (`spans` is a host array of device pointers, any alignment); out_device: one cfhip_lz_stats on the
 * device, 8-byte aligned, overwritten.  The stream rules of cfhip_compare_device. */
int cfhip_lz_size_device(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, cfhip_lz_stats* out_device,
	void* stream);

/* The two entries below are diagnostic: they serve the tests and tools/bench_lzsize.py, are not needed to use the
 * estimator, and may change without a new CFHIP_ABI_VERSION.
 *
 * A stream longer than a slice is processed in slices, each behind the 32768 bytes before it; the result does not
 * depend on the slice.  Sets the slice (rounded up to whole blocks of 65536 bytes; 0 = the default, 4 MiB) and
 * returns the one in force before.  It bounds the context's scratch. */
size_t cfhip_lz_slice_bytes(cfhip_ctx* ctx, size_t bytes);

/* Kernel time of the five stages (keys, sort, match, parse, cost) of the estimate the most recent call on this
 * context made last, summed over its slices (ms); CFHIP_E_INVALID unless that call was a cfhip_lz_size*.
 * Synchronises the stream. */
int cfhip_lz_stage_ms(cfhip_ctx* ctx, float ms[5]);

/* ---- the zlib stream of payloads (csrc/deflate.hip) ----
 * The real encoder behind the estimate: the stream (the spans of a call, concatenated; fewer than 2^31 bytes) becomes
 * one zlib stream (RFC 1950 around RFC 1951) that any inflate reads back.  The tokens are exactly those cfhip_lz_size
 * prices -- same candidates, same parse, same 4096-byte chunks -- so literals, matches and matched_bytes equal its.
 * Every 65536 input bytes form a group that starts on a byte boundary and takes the smallest of three forms: stored
 * blocks, the fixed codes, or its own length-limited Huffman codes (15 bits; 7 for the code-length code) with the
 * code-table header; a coded group ends in an empty stored block.  The definition, byte for byte, is
 * tests/deflate_ref.py; identical calls return identical bytes, whatever the slice (cfhip_lz_slice_bytes governs this
 * path too).  Scratch belongs to the context: about 21.4 bytes per byte of a slice. */
typedef struct cfhip_deflate_result {
	uint64_t bytes_in, bytes_out;                           /* bytes of the stream, bytes written */
	uint64_t blocks_stored, blocks_fixed, blocks_dynamic;   /* groups per form */
	uint64_t literals, matches, matched_bytes;              /* cfhip_lz_stats' */
	uint32_t adler32, reserved;                             /* the stream's Adler-32; 0 */
} cfhip_deflate_result;

/* Bytes that hold the zlib stream of any n input bytes: 11 + n + 10 per started group of 65536.  Needs no device. */
size_t cfhip_deflate_bound(size_t n);

/* Host spans and a host buffer of `cap` bytes; cap < cfhip_deflate_bound(bytes of the stream) is CFHIP_E_CAPACITY,
 * 2^31 bytes or more too.  Bytes of `out` past result->bytes_out are unspecified.  A span of 0 bytes is skipped; a
 * stream of 0 bytes is CFHIP_OK with the 11-byte stream of an empty input and needs no context.  Every argument is
 * checked before anything is enqueued (a NULL ctx is reported last).  Blocking. */
int cfhip_deflate(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out, size_t cap,
	cfhip_deflate_result* result);

/* Device spans (a host array of device pointers, any alignment); out_device: `cap` bytes on the device, 4-byte aligned,
 * overwritten up to cfhip_deflate_bound; result_device: one cfhip_deflate_result on the device, 8-byte aligned.
 * The stream rules of cfhip_compare_device. */
int cfhip_deflate_device(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out_device, size_t cap,
	cfhip_deflate_result* result_device, void* stream);

/* The two entries below are diagnostic, like cfhip_lz_stage_ms.
 *
 * Kernel time of the eight stages (keys, sort, match, parse, adler, codes, offsets, emit) of the most recent call on
 * this context, summed over its slices (ms); CFHIP_E_INVALID unless that call was a cfhip_deflate*.  Synchronises. */
int cfhip_deflate_stage_ms(cfhip_ctx* ctx, float ms[8]);

/* The device code builder alone: the code lengths (at most `limit` <= 15 bits, 2 <= n <= 288 <= 2^limit symbols) of a
 * histogram in host memory, by the rule of tests/deflate_ref.py code_lengths: fewer than two used symbols are made two,
 * the lengths' Kraft sum is exactly 1.  Blocking. */
int cfhip_deflate_code_lengths(cfhip_ctx* ctx, const uint32_t* counts, uint32_t n, uint32_t limit, uint8_t* lengths);

/* ---- indexed zlib streams and their inflate (csrc/inflate.hip, csrc/inflate.h) ----
 * A zlib stream is serial; with a small side index every 4096 output bytes of it decode on their own.  Bits are numbered
 * from the start of the zlib stream: bit k is bit k & 7 of byte k >> 3.  For a stream whose output is n bytes the index
 * has ceil(n / 4096) entries.  A stream is indexable when every output position 4096 c is the first byte of a token:
 * every stream of cfhip_deflate is, and so is any stream flushed (Z_SYNC_FLUSH) after every 4096 input bytes.  The index
 * is a pure function of the stream; its definition, and that of everything below, is tests/inflate_ref.py. */
typedef struct cfhip_zindex_entry {
	uint64_t header_bit;  /* the BFINAL bit of the deflate block that holds output byte 4096*c */
	uint64_t token_bit;   /* first bit of the literal/length code of the token that produces that byte;
	                         in a stored block: 8 * the position of that data byte */
} cfhip_zindex_entry;

/* ceil(n / 4096).  Needs no device. */
size_t cfhip_zindex_entries(size_t n);

/* cfhip_deflate / cfhip_deflate_device with the stream's index: the same bytes and the same result for the same spans,
 * and entry c of `index` (host memory / device memory, 8-byte aligned) for every 4096 bytes of the spans.
 * index_entries < cfhip_zindex_entries(bytes of the spans) is CFHIP_E_CAPACITY, checked with the other arguments
 * before anything is enqueued. */
int cfhip_deflate_indexed(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out, size_t cap,
	cfhip_zindex_entry* index, size_t index_entries, cfhip_deflate_result* result);
int cfhip_deflate_indexed_device(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out_device, size_t cap,
	cfhip_zindex_entry* index_device, size_t index_entries, cfhip_deflate_result* result_device, void* stream);

/* The error classes of cfhip_inflate_result.status.  Which defect yields which class, and in what order a chunk
 * notices them, is defined by tests/inflate_ref.py inflate_indexed; the kernels return its (status, bad_chunk). */
enum cfhip_inflate_status {
	CFHIP_INFLATE_OK = 0,
	CFHIP_INFLATE_WRAPPER = 1,    /* CMF / FLG, or the stream is not exactly zbytes long */
	CFHIP_INFLATE_INDEX = 2,      /* an entry is not where the stream's tokens are, or the stream holds more than out_bytes */
	CFHIP_INFLATE_HEADER = 3,     /* a block header */
	CFHIP_INFLATE_CODE = 4,       /* a bit pattern of no code, symbols 286 / 287, distance codes 30 / 31 */
	CFHIP_INFLATE_DISTANCE = 5,   /* a distance that reaches before output byte 0 */
	CFHIP_INFLATE_OVERRUN = 6,    /* the stream, or its BFINAL block, ends before the output does */
	CFHIP_INFLATE_CHECKSUM = 7    /* the Adler-32 of the output is not the trailer's */
};

typedef struct cfhip_inflate_result {
	uint64_t bytes_in, bytes_out;                /* bytes of the zlib stream; bytes written (0 unless status is 0) */
	uint64_t literals, matches, matched_bytes;   /* of the tokens read (a stored byte is a literal): cfhip_deflate_result's
	                                                for our own streams without stored groups; 0 unless status is 0 */
	uint32_t adler32, status, bad_chunk, rounds; /* computed Adler-32; 0 or an error class; lowest failing chunk; resolve rounds run */
} cfhip_inflate_result;

/* The out_bytes bytes of an indexed zlib stream of exactly zbytes bytes (out_bytes is the expected size; fewer than
 * 2^31, zbytes at most 2^32).  Every chunk of 4096 output bytes decodes from its entry on its own wavefront and checks
 * that it arrives exactly at the next entry; chunk 0 checks the link from bit 16, the last chunk the end of the stream:
 * the index is validated, not trusted, and a stream that passes is a valid zlib stream whose output is what was written.
 * The rules of the format.  Wrapper: the low four bits of CMF are 8, FCHECK is valid, no FDICT, and the stream is
 * exactly zbytes long (after the BFINAL block the padding bits, the big-endian Adler-32, nothing).  A dynamic header
 * is rejected when HLIT > 286 or HDIST > 30, when a repeat code comes first or a run goes past HLIT + HDIST, when
 * symbol 256 has length 0, or when one of the three codes has a Kraft sum above 1; an incomplete code is accepted.  A
 * bit pattern that belongs to no code, literal/length symbols 286 and 287 and distance codes 30 and 31 are code
 * errors; a distance that reaches before output byte 0 is a distance error.
 * Returns CFHIP_E_DATA for a stream that fails, with *result filled and the class and chunk in cfhip_last_error; the
 * contents of `out` are then unspecified.  Nothing outside [out, out + out_bytes) is ever written.
 * index_entries < cfhip_zindex_entries(out_bytes) is CFHIP_E_CAPACITY; every argument is checked before anything is
 * enqueued (a NULL ctx is reported last).  out_bytes == 0 needs no context.  `rounds` is the depth of the longest copy
 * chain inside one slice (cfhip_lz_slice_bytes): the one field that depends on the slice.  Scratch belongs to the
 * context: 8 bytes per byte of a slice.  Blocking. */
int cfhip_inflate(cfhip_ctx* ctx, const void* zstream, size_t zbytes, const cfhip_zindex_entry* index,
	size_t index_entries, void* out, size_t out_bytes, cfhip_inflate_result* result);

/* Everything on the device: index_device and result_device 8-byte aligned, out_device 4-byte aligned.  Returns CFHIP_OK
 * once enqueued; an invalid stream is reported through result_device->status.  The stream rules of
 * cfhip_compare_device. */
int cfhip_inflate_device(cfhip_ctx* ctx, const void* zstream_device, size_t zbytes, const cfhip_zindex_entry* index_device,
	size_t index_entries, void* out_device, size_t out_bytes, cfhip_inflate_result* result_device, void* stream);

/* Diagnostic: kernel time of the four stages (decode, resolve, pack, fold) of the most recent call on this context,
 * summed over its slices (ms); CFHIP_E_INVALID unless that call was a cfhip_inflate*.  Synchronises. */
int cfhip_inflate_stage_ms(cfhip_ctx* ctx, float ms[4]);

/* ---- LZ4 frames of payloads, both ways (csrc/lz4.hip, csrc/lz4.h) ----
 * The fast-to-load companion of the rate-distortion pass, not a replacement for cfhip_deflate: LZ4 has no entropy
 * stage, so plain payloads barely shrink and payloads after cfhip_rdo* do (DESIGN.md section 4.18 has the figures).
 * The stream (the spans of a call, concatenated; fewer than 2^31 bytes) becomes ONE LZ4 frame (LZ4 Frame Format 1.6)
 * that the lz4 tool and liblz4's LZ4F_decompress read: version 01, independent blocks of 64 KiB, block checksums,
 * content size, no content checksum, no dictionary id.  The tokens of a block are cfhip_lz_size's on that block
 * taken as a stream of its own; adjacent matches of one distance are merged, the block format's end rules applied,
 * and a block that does not shrink is stored raw.  The definition, byte for byte, is tests/lz4_ref.py; identical
 * calls return identical bytes, whatever the slice (cfhip_lz_slice_bytes).  Scratch belongs to the context: about 27
 * bytes per byte of a slice. */
typedef struct cfhip_lz4_result {
	uint64_t bytes_in, bytes_out;                  /* bytes of the stream, bytes of the frame */
	uint64_t blocks_compressed, blocks_stored;
	uint64_t sequences, literals, matched_bytes;   /* over the compressed blocks; each block's last, literal-only
	                                                  sequence is counted */
} cfhip_lz4_result;

/* Bytes that hold the frame of any n input bytes: 19 + n + 8 per started block of 65536.  Needs no device. */
size_t cfhip_lz4_bound(size_t n);

/* The argument rules of cfhip_deflate: cap < cfhip_lz4_bound(bytes of the stream) is CFHIP_E_CAPACITY, 2^31 bytes or
 * more too; a stream of 0 bytes is CFHIP_OK with the 19-byte frame of an empty input and needs no context; every
 * argument is checked before anything is enqueued (a NULL ctx is reported last).  Blocking. */
int cfhip_lz4_encode(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out, size_t cap,
	cfhip_lz4_result* result);

/* Device spans; out_device: `cap` bytes on the device, overwritten up to cfhip_lz4_bound; result_device: one
 * cfhip_lz4_result on the device, 8-byte aligned.  The stream rules of cfhip_compare_device. */
int cfhip_lz4_encode_device(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out_device, size_t cap,
	cfhip_lz4_result* result_device, void* stream);

/* Diagnostic: kernel time of the first n <= 9 stages (keys, sort, match, parse, plan, offsets, emit, hash, final) of the
 * most recent call on this context, summed over its slices (ms); CFHIP_E_INVALID unless that call was a
 * cfhip_lz4_encode*.  Synchronises. */
int cfhip_lz4_encode_stage_ms(cfhip_ctx* ctx, float* ms, size_t n);

/* The classes of cfhip_lz4_decode_result.status.  Which defect yields which class, and in what order a block notices
 * them, is defined by tests/lz4_ref.py decode; the kernels return its (status, bad_block). */
enum cfhip_lz4_status {
	CFHIP_LZ4_OK = 0,
	CFHIP_LZ4_HEADER = 1,        /* magic, version, reserved bits, a block-size code below 4, HC, a frame shorter than its header */
	CFHIP_LZ4_UNSUPPORTED = 2,   /* a valid header this decoder does not take: linked blocks, blocks above 64 KiB, a dictionary id */
	CFHIP_LZ4_BLOCKS = 3,        /* the size chain leaves the stream, a size above 65536 or a raw size of 0, no end mark, trailing bytes */
	CFHIP_LZ4_CHECKSUM = 4,      /* a block's XXH32 is not the one stored behind it */
	CFHIP_LZ4_SEQUENCE = 5,      /* a literal run or a match leaves the block's input or its output; a truncated sequence */
	CFHIP_LZ4_OFFSET = 6,        /* an offset of 0, or one that reaches before the block's first byte */
	CFHIP_LZ4_SIZE = 7           /* the content size is not out_bytes; a block does not decode to its share of out_bytes */
};

typedef struct cfhip_lz4_decode_result {
	uint64_t bytes_in, bytes_out;                  /* bytes of the frame; bytes written (0 unless status is 0) */
	uint64_t blocks_compressed, blocks_stored;     /* cfhip_lz4_result's for our own frames; 0 unless status is 0 */
	uint64_t sequences, literals, matched_bytes;
	uint32_t status, bad_block;                    /* 0 or a class; the lowest failing block (the number of blocks: the frame's end) */
	uint32_t content_checksum, reserved;           /* 1: the frame carries a content checksum, which was NOT verified; 0 */
} cfhip_lz4_decode_result;

/* The out_bytes bytes (the expected size; fewer than 2^31) of exactly one LZ4 frame of exactly `bytes` bytes, anyone's:
 * version 01, independent blocks, 64 KiB maximum block size, no dictionary id; block checksums and the content size
 * are verified where present, a content checksum may be present and is skipped (XXH32 is one serial chain over the
 * whole output); every block but the last decodes to exactly 65536 bytes.  One wavefront decodes one block.  The frame
 * is validated, not trusted: every length is range-checked before use, nothing outside the frame is read, nothing
 * outside [out, out + out_bytes) is written.  Returns CFHIP_E_DATA for a frame that fails, with *result filled and the
 * class and block in cfhip_last_error; the contents of `out` are then unspecified.  Every argument is checked before
 * anything is enqueued (a NULL ctx is reported last); out_bytes == 0 needs no context.  Blocking. */
int cfhip_lz4_decode(cfhip_ctx* ctx, const void* frame, size_t bytes, void* out, size_t out_bytes,
	cfhip_lz4_decode_result* result);

/* Everything on the device: out_device 4-byte aligned, result_device 8-byte aligned, frame_device any alignment.
 * Returns CFHIP_OK once enqueued; an invalid frame is reported through result_device->status.  The stream rules of
 * cfhip_compare_device. */
int cfhip_lz4_decode_device(cfhip_ctx* ctx, const void* frame_device, size_t bytes, void* out_device, size_t out_bytes,
	cfhip_lz4_decode_result* result_device, void* stream);

/* Diagnostic: kernel time of the first n <= 3 stages (chain, blocks, final) of the most recent call on this context
 * (ms); CFHIP_E_INVALID unless that call was a cfhip_lz4_decode*.  Synchronises. */
int cfhip_lz4_decode_stage_ms(cfhip_ctx* ctx, float* ms, size_t n);

/* ---- PNG files of images (csrc/png.hip, csrc/png.h) ----
 * Image::save for the .png extension with the texels on the device: one file of signature, IHDR, an sRGB chunk
 * (rendering intent 0) when color_space is CFHIP_COLOR_SRGB, exactly one IDAT chunk holding one zlib stream, IEND.
 * color_type 0 (grey), 2 (RGB), 4 (grey + alpha) or 6 (RGBA) at bit_depth 8 or 16; no interlace.  The source is RGBA8,
 * RGBA16F or RGBA32F with a row pitch.  Samples: floats as the encoders quantise them, round(clamp(f, 0, 1) x 255) or
 * x 65535, computed in float, NaN -> 0; an RGBA8 source at depth 16 is widened by v x 257; grey takes the red channel;
 * colour types without alpha drop it; 16-bit samples are big-endian.  Every row gets the filter type, 0 to 4, with the
 * smallest sum over its filtered bytes of (b < 128 ? b : 256 - b), the lowest type winning a tie (the PNG
 * specification's heuristic); filters read the raw row above, zeros above the first.  The zlib stream is cfhip_deflate's
 * of the filtered bytes, height x (1 + row bytes) of them, fewer than 2^31.  The definition, byte for byte, is
 * tests/png_ref.py; identical calls return identical bytes and result bits.  Not written: palette, sub-byte and
 * interlaced images (CFHIP_E_UNSUPPORTED), ancillary chunks other than sRGB.  Scratch belongs to the context: about 2
 * bytes per filtered byte beside the deflate encoder's. */
typedef struct cfhip_png_result {
	uint64_t bytes_out, idat_bytes, filtered_bytes;   /* bytes of the file, of the IDAT data (the zlib stream), of its input */
	uint32_t rows_by_filter[5];                       /* rows per filter type: None, Sub, Up, Average, Paeth */
	uint32_t idat_crc32;                              /* the IDAT chunk's CRC */
	cfhip_deflate_result deflate;                     /* the zlib stream's */
} cfhip_png_result;

/* Bytes that hold the file of any such image: 8 + 25 + (sRGB ? 13 : 0) + 12 + cfhip_deflate_bound(height x (1 + row
 * bytes)) + 12.  0 for a zero size, and for a colour type, depth or colour space the calls below do not take.  Needs no
 * device. */
size_t cfhip_png_bound(uint32_t width, uint32_t height, int color_type, int bit_depth, int color_space);

/* Host buffers.  pixels: rows pitch_bytes apart (>= width x the texel's bytes).  The argument rules of cfhip_deflate:
 * every argument is checked before anything is enqueued, in this order -- out, result, pixels NULL; a zero width or
 * height (CFHIP_E_INVALID); the pixel type; the colour space; colour type 3 (CFHIP_E_UNSUPPORTED) or unknown; depth 1,
 * 2 or 4 (CFHIP_E_UNSUPPORTED) or unknown; the pitch; 2^31 filtered bytes or more, then cap < cfhip_png_bound
 * (CFHIP_E_CAPACITY); a NULL ctx last.  Nothing outside [out, out + cap) is written; bytes past result->bytes_out are
 * unspecified.  Blocking. */
int cfhip_png_encode(cfhip_ctx* ctx, const void* pixels, int pixel_type, size_t pitch_bytes, uint32_t width,
	uint32_t height, int color_type, int bit_depth, int color_space, void* out, size_t cap, cfhip_png_result* result);

/* Everything on the device: pixels_device and pitch_bytes aligned to the texel's size (4, 8 or 16 bytes), out_device
 * any alignment (where the IDAT data, 41 or 54 bytes in, falls on a 4-byte boundary the stream is written in place;
 * otherwise the CRC kernel moves it there), result_device 8-byte aligned.  The stream rules of cfhip_compare_device. */
int cfhip_png_encode_device(cfhip_ctx* ctx, const void* pixels_device, int pixel_type, size_t pitch_bytes,
	uint32_t width, uint32_t height, int color_type, int bit_depth, int color_space, void* out_device, size_t cap,
	cfhip_png_result* result_device, void* stream);

/* Diagnostic, like cfhip_lz4_encode_stage_ms: kernel time of the eleven stages (filter; keys, sort, match, parse, adler,
 * codes, offsets, emit of the zlib encoder, summed over its slices; crc; final) of the most recent call on this context
 * (ms); CFHIP_E_INVALID unless that call was a cfhip_png_encode*.  Synchronises. */
int cfhip_png_stage_ms(cfhip_ctx* ctx, float ms[11]);

/* The pass to a target: the smallest lambda whose result is estimated at no more than
 * T = floor(target_ratio * est_bytes_plain), est_bytes_plain being the estimate of the payloads as given.  The stream
 * is the surfaces' payloads concatenated in call order.  params->lambda is the largest lambda allowed:
 * hi = round(16 lambda); the pass runs at hi from the pristine payloads; if its estimate exceeds T that result is
 * returned with reached = 0.  Otherwise lo = 0 and, while hi - lo > 1, mid = (lo + hi) / 2 is tried: hi = mid if its
 * estimate is <= T, else lo = mid; the pass at hi is returned with reached = 1.  Every trial starts from the pristine
 * payloads (kept in the context's scratch where out == blocks).  stats are those of the returned pass; flags, cap,
 * mask and window are cfhip_rdo_ex's, as are the checks; target_ratio outside (0, 1) is CFHIP_E_INVALID.  No host
 * compressor runs.  Both forms block: each trial's estimate is read back before the next one is chosen. */
typedef struct cfhip_rdo_target_result {
	uint32_t lambda16;          /* round(16 lambda) of the returned pass */
	uint32_t reached;           /* 1: est_bytes_final <= T */
	uint32_t trials;            /* passes estimated during the search */
	uint64_t est_bytes_plain, est_bytes_final;
} cfhip_rdo_target_result;

int cfhip_rdo_target(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n_surfaces,
	const cfhip_rdo_ex_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats, float target_ratio,
	cfhip_rdo_target_result* result);

/* The buffers of cfhip_rdo_ex_device; result is host memory. */
int cfhip_rdo_target_device(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n_surfaces,
	const cfhip_rdo_ex_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats_device, float target_ratio,
	cfhip_rdo_target_result* result, void* stream);

/* ---- PVRTC1 4 bpp (formats 59 RGB, 60 RGBA; type UNorm) ----
 *
 * PVRTC1 is outside the cfhip_surface block contract: blocks are stored in twiddled (Morton) order, a level is never
 * smaller than 2 x 2 blocks, sizes must be powers of two, and every texel blends the colours of four blocks with
 * wrap-around.  So it has its own entries.  Payload of a w x h level: max(w/4, 2) * max(h/4, 2) * 8 bytes; a surface
 * under 8 texels repeats itself (texel (x mod w, y mod h)) in the encoder.  The decoded layout is RGBA8 (alpha 255 for
 * the RGB format). */

/* Payload bytes of a w x h level.  CFHIP_E_UNSUPPORTED for every format but 59 / 60 and for types other than UNorm;
 * CFHIP_E_INVALID for sizes that are not powers of two (or above 32768).  Pure, needs no device. */
int cfhip_pvrtc_query(int format, int type, uint32_t width, uint32_t height, size_t* bytes);

/* Encode with the cfhip_surface / cfhip_params of cfhip_encode: same pixel types and pitch rules, negative pitch
 * included (|pitch| a multiple of the pixel size); out_capacity >= the cfhip_pvrtc_query size.  RGBA32F / RGBA16F
 * are quantised as the host pipeline quantises them (toColorBlock).  mask_rgba weights the channels of the error.
 * One launch per pass for all surfaces of the call.  Blocking.  The device form takes device pointers and the
 * stream rules of cfhip_encode_device; both produce identical payloads. */
int cfhip_pvrtc_encode(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n_surfaces,
	const cfhip_params* params);
int cfhip_pvrtc_encode_device(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n_surfaces,
	const cfhip_params* params, void* stream);

/* Decode to RGBA8 rows (the cfhip_decode rules; device buffers 4-byte aligned). */
int cfhip_pvrtc_decode(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes,
	uint32_t width, uint32_t height, void* out, size_t out_capacity);
int cfhip_pvrtc_decode_device(cfhip_ctx* ctx, int format, int type, const void* blocks, uint32_t width,
	uint32_t height, void* out, size_t out_pitch_bytes, void* stream);
/* Decode and compare against an RGBA8 reference in one pass: exact per-channel sums of squared differences (the
 * cfhip_decode_sse rules).  The device form's sse_device (four uint64, zeroed by the call on the stream) must be
 * 8-byte aligned; otherwise CFHIP_E_INVALID, nothing enqueued. */
int cfhip_pvrtc_decode_sse(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes,
	uint32_t width, uint32_t height, const void* ref_rgba8, size_t ref_pitch_bytes, uint64_t sse[4]);
int cfhip_pvrtc_decode_sse_device(cfhip_ctx* ctx, int format, int type, const void* blocks, uint32_t width,
	uint32_t height, const void* ref_rgba8, size_t ref_pitch_bytes, uint64_t* sse_device, void* stream);

/* ---- Standard (uncompressed) formats 1..28: the payload back to texels, and its quality metrics ----
 *
 * The inverse of what cfhip_encode writes for these formats: width * height pixels, row-major, top-down, tightly
 * packed -> RGBA32F texels.  Legality is cfhip_query's for formats 1..28 (66 pairs); every other (format, type) --
 * block formats, PVRTC, illegal pairs such as (R5G6B5, Float) -- is CFHIP_E_UNSUPPORTED.  The generic
 * cfhip_decode* / cfhip_compare* entries keep answering CFHIP_E_UNSUPPORTED for these formats.
 *
 * Value of a stored field v of n bits (the fixed-function conversions of Vulkan / OpenGL):
 *   UNorm               (float)v / (float)(2^n - 1), the correctly rounded IEEE single division
 *   SNorm               max((float)v / (float)(2^(n-1) - 1), -1.0f), v sign-extended
 *   UInt / Int          (float)v, round to nearest even (exact up to 2^24)
 *   Float, 16-bit       half -> float, exact
 *   Float, 32-bit       the stored bits, copied
 *   UFloat B10G11R11    unsigned small floats, exponent bias 15, 6 / 6 / 5 mantissa bits; exponent 0 is a denormal
 *                       m * 2^(-14 - mbits); exponent 31 is +Inf (m == 0) or NaN
 *   UFloat E5B9G9R9     m_c * 2^(e - 24) per channel, exact in float
 * Channels the format does not store: green and blue 0, alpha 1.  A stored NaN stays a NaN; its bits are not
 * specified, except for 32-bit Float, whose bits are copied.  Colour space: the stored values are returned, no
 * sRGB transfer is applied.
 *
 * Stream and error rules are those of cfhip_decode*: every argument is checked before anything is enqueued,
 * stream == NULL means the context's stream and the call synchronises. */

/* Host buffers: pixels (pixels_bytes >= width * height * pixel size) -> out_rgba32f, width * height texels tightly
 * packed (out_capacity >= width * height * 16 bytes, else CFHIP_E_CAPACITY).  Blocking. */
int cfhip_std_unpack(cfhip_ctx* ctx, int format, int type, const void* pixels, size_t pixels_bytes,
	uint32_t width, uint32_t height, void* out_rgba32f, size_t out_capacity);

/* Device buffers on ctx's GPU.  pixels may have any alignment (a mip level inside a larger payload).  out_rgba32f:
 * rows out_pitch_bytes apart (>= width * 16); pointer and pitch 4-byte aligned (16 for the fastest stores). */
int cfhip_std_unpack_device(cfhip_ctx* ctx, int format, int type, const void* pixels,
	uint32_t width, uint32_t height, void* out_rgba32f, size_t out_pitch_bytes, void* stream);

/* cfhip_compare for the standard formats: every pixel is converted as above (to the float cfhip_std_unpack writes,
 * then to double) and measured against the reference exactly as cfhip_compare measures a decoded block texel.
 * Channels compared: those the format stores AND the caller's mask; the others report 0 (ssim NaN).
 *   sse, ref_max   every type
 *   log_sse        Float and UFloat types (NaN otherwise)
 *   ssim           with CFHIP_COMPARE_SSIM, UNorm (L = 1) and SNorm (L = 2) types; NaN for the other types, when
 *                  not asked for and when a side is below 11
 * error_blocks is 0 and there is no per-block error map.  Identical calls return identical bits. */
int cfhip_std_compare(cfhip_ctx* ctx, int format, int type, const void* pixels, size_t pixels_bytes,
	uint32_t width, uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch_bytes,
	const uint8_t mask_rgba[4], unsigned flags, cfhip_compare_result* result);

/* Device buffers: pixels (any alignment), ref (pointer and pitch aligned to the texel size), result_device (8-byte
 * aligned).  mask_rgba is host memory.  The stream rules of cfhip_compare_device. */
int cfhip_std_compare_device(cfhip_ctx* ctx, int format, int type, const void* pixels,
	uint32_t width, uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch_bytes,
	const uint8_t mask_rgba[4], unsigned flags, cfhip_compare_result* result_device, void* stream);

/* Kernel-only time of the most recent cfhip_encode, cfhip_encode_device, cfhip_pvrtc_*, cfhip_decode*, cfhip_compare*, cfhip_std_*, cfhip_rdo* (every trial of cfhip_rdo_target*), cfhip_lz_size*, cfhip_deflate*, cfhip_png_encode* (the filter, the encoder's stages, crc and final), cfhip_image_ops_device, cfhip_mip_post_array_device (every launch of the post-pass), cfhip_alpha_coverage_device, cfhip_alpha_bleed_array_device, cfhip_alpha_sdf_array_device (every pass), cfhip_spec_aa_array_device (every launch), cfhip_height_ao_array_device (both launches), cfhip_equirect_to_cube_device, cfhip_cube_prefilter_device (every level), cfhip_cube_sh9_device (both launches), cfhip_brdf_lut_device or cfhip_cube_irradiance_device call on
 * this context, measured with hipEvents on the launch stream (ms; <0 if none).
 * Synchronises the stream. */
float cfhip_last_kernel_ms(cfhip_ctx* ctx);

/* Accumulate kernel timings over several calls: between cfhip_profile_begin and
 * cfhip_profile_end every launch made through this context is bracketed by
 * hipEvents on its launch stream.  _end synchronises, returns the summed kernel
 * time (ms) and the number of launches. */
int cfhip_profile_begin(cfhip_ctx* ctx);
int cfhip_profile_end(cfhip_ctx* ctx, float* total_ms, uint32_t* launches);

/* Page-locked host memory this context holds for its host path right now (bytes): the three source strip slots and
 * the landing ring of the payload (four strips) -- independent of the size of the surfaces it has converted. */
size_t cfhip_pinned_bytes(const cfhip_ctx* ctx);

/* Name of the kernel that dominated the last call (for rocprof cross-reference). */
const char* cfhip_last_kernel_name(const cfhip_ctx* ctx);

const char* cfhip_last_error(const cfhip_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* CUTTLEFISH_HIP_H */
