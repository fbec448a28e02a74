// png.h -- what the host side (cfhip_api.hip), the kernels (png.hip) and the host program (tools/png_host.cpp) of the PNG
// writer share: the constants of the format, the sample rule, the five filters and their cost, CRC-32 with the algebra
// that combines pieces of it, the bytes around the IDAT data, the bound -- and, for the device side, the scratch layout
// and the launchers.
// The definition of every byte is tests/png_ref.py.  Everything above the __HIPCC__ part
// compiles with the host compiler alone.
//
// Scratch of a call (the context's, grown on demand): the filtered bytes, a zlib stream's bound where the stream cannot
// be written in place (the IDAT data starts 41 or 54 bytes into the file and cfhip_deflate_device wants 4-byte
// alignment) and 256 bytes of state: about 2 bytes per filtered byte, beside the deflate encoder's own (deflate.h).
#ifndef CF_PNG_H
#define CF_PNG_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CFPNG_FN __host__ __device__ inline
#else
#define CFPNG_FN inline
#endif

#define CFPNG_GREY 0
#define CFPNG_RGB 2
#define CFPNG_PALETTE 3
#define CFPNG_GREY_ALPHA 4
#define CFPNG_RGBA 6
#define CFPNG_FILTERS 5             // None, Sub, Up, Average, Paeth
#define CFPNG_POLY 0xEDB88320u      // the IEEE polynomial, reflected
#define CFPNG_SUB 64u               // bytes of which one lane takes the CRC
#define CFPNG_SUBS 256u             // ... of a workgroup's piece: 16 KiB
#define CFPNG_TAIL 16u              // the IDAT CRC and IEND
// The pixel types of the source (cuttlefish_hip.h: enum cfhip_pixel_type).
#define CFPNG_PIX_RGBA8 0
#define CFPNG_PIX_RGBA32F 1
#define CFPNG_PIX_RGBA16F 2
// The timed stages of a call: filter, the zlib encoder's eight (deflate.h), crc, final.
#define CFPNG_STAGES 11
// The state of a call (uint32 words), zeroed before the first kernel.
#define CFPNG_S_ROWS 0              // [5] rows per filter type
#define CFPNG_S_CRC 5               // XOR of the pieces' shares of the IDAT CRC register
#define CFPNG_S_DEFLATE 8           // cfhip_deflate_result: nine 64-bit words, 8-byte aligned
#define CFPNG_S_WORDS 64

// ---- geometry ------------------------------------------------------------------------------------------------------
CFPNG_FN uint32_t cfpng_channels(int color_type)
{
	return color_type == CFPNG_GREY ? 1u : color_type == CFPNG_GREY_ALPHA ? 2u : color_type == CFPNG_RGB ? 3u :
		color_type == CFPNG_RGBA ? 4u : 0u;
}

// bytes per pixel: 1, 2, 3, 4, 6 or 8 (0: not a colour type / depth written here)
CFPNG_FN uint32_t cfpng_bpp(int color_type, int bit_depth)
{
	return (bit_depth == 8 || bit_depth == 16) ? cfpng_channels(color_type)*(uint32_t)bit_depth/8u : 0u;
}

// height x (1 + row bytes), saturating
CFPNG_FN uint64_t cfpng_filtered_bytes(uint32_t width, uint32_t height, uint32_t bpp)
{
	const uint64_t row = 1u + (uint64_t)width*bpp;
	return height && row > UINT64_MAX/height ? UINT64_MAX : row*height;
}

// cfhip_deflate_bound (deflate.h: cfdf_bound)
CFPNG_FN uint64_t cfpng_zlib_bound(uint64_t n)
{
	return 11u + n + 10u*((n + 65535u)/65536u);
}

CFPNG_FN uint32_t cfpng_data_offset(int srgb)
{
	return 8u + 25u + (srgb ? 13u : 0u) + 8u;
}

// 8 + 25 + (sRGB ? 13 : 0) + 12 + cfhip_deflate_bound(filtered bytes) + 12; 0 for an image this writer does not take
CFPNG_FN uint64_t cfpng_bound(uint32_t width, uint32_t height, int color_type, int bit_depth, int srgb)
{
	const uint32_t bpp = cfpng_bpp(color_type, bit_depth);
	if (!bpp || !width || !height)
		return 0u;
	const uint64_t n = cfpng_filtered_bytes(width, height, bpp);
	if (n >= ((uint64_t)1 << 62))
		return UINT64_MAX;
	return cfpng_data_offset(srgb) + cfpng_zlib_bound(n) + CFPNG_TAIL;
}

// ---- samples -------------------------------------------------------------------------------------------------------
// round(clamp(f, 0, 1) x 255), NaN -> 0: cf_unorm8's rule (cf_device.h) with the NaN case spelled out
CFPNG_FN uint32_t cfpng_q8(float f)
{
	f = f > 0.0f ? (f < 1.0f ? f : 1.0f) : 0.0f;
	return (uint32_t)roundf(f*255.0f);
}

CFPNG_FN uint32_t cfpng_q16(float f)
{
	f = f > 0.0f ? (f < 1.0f ? f : 1.0f) : 0.0f;
	return (uint32_t)roundf(f*65535.0f);
}

// binary16 -> binary32, exact
CFPNG_FN float cfpng_half(uint32_t h)
{
	const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
	uint32_t bits;
	if (e == 31u)
		bits = sign | 0x7F800000u | (m << 13);
	else if (e)
		bits = sign | ((e + 112u) << 23) | (m << 13);
	else {
		// a subnormal is m x 2^-24: exact in binary32
		float f = (float)m*(1.0f/16777216.0f);
		uint32_t fb;
		memcpy(&fb, &f, 4);
		bits = sign | fb;
	}
	float out;
	memcpy(&out, &bits, 4);
	return out;
}

// The sample of channel c (0 red .. 3 alpha) of one source texel given as its 32-bit words: 8 or 16 bits.
template <int PIX, int D16>
CFPNG_FN uint32_t cfpng_sample(const uint32_t w[4], uint32_t c)
{
	if (PIX == CFPNG_PIX_RGBA8) {
		const uint32_t v = (w[0] >> (8u*c)) & 255u;
		return D16 ? v*257u : v;
	}
	float f;
	if (PIX == CFPNG_PIX_RGBA32F)
		memcpy(&f, &w[c], 4);
	else
		f = cfpng_half((w[c >> 1] >> (16u*(c & 1u))) & 0xFFFFu);
	return D16 ? cfpng_q16(f) : cfpng_q8(f);
}

// The raw bytes of one pixel in file order, byte 0 in bits 0..7: CH channels (1 red, 2 red + alpha, 3 RGB, 4 RGBA),
// 16-bit samples big-endian.
template <int PIX, int CH, int D16>
CFPNG_FN uint64_t cfpng_pixel(const uint32_t w[4])
{
	uint64_t px = 0u;
	for (uint32_t k = 0; k < (uint32_t)CH; ++k) {
		const uint32_t c = (CH == 2 && k == 1u) ? 3u : k;
		const uint32_t s = cfpng_sample<PIX, D16>(w, c);
		if (D16)
			px |= (uint64_t)(((s >> 8) & 255u) | ((s & 255u) << 8)) << (16u*k);
		else
			px |= (uint64_t)s << (8u*k);
	}
	return px;
}

// ---- filters (PNG specification, section 9) ------------------------------------------------------------------------
CFPNG_FN uint32_t cfpng_paeth(uint32_t a, uint32_t b, uint32_t c)
{
	const int p = (int)a + (int)b - (int)c;
	const int pa = p > (int)a ? p - (int)a : (int)a - p;
	const int pb = p > (int)b ? p - (int)b : (int)b - p;
	const int pc = p > (int)c ? p - (int)c : (int)c - p;
	return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// x: the byte; a: bpp bytes back; b: above; c: above a -- all raw
CFPNG_FN uint32_t cfpng_filter(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
	const uint32_t pred = type == 0u ? 0u : type == 1u ? a : type == 2u ? b : type == 3u ? (a + b) >> 1 : cfpng_paeth(a, b, c);
	return (x - pred) & 255u;
}

// what a filtered byte costs in the heuristic: its distance from 0 as a signed byte
CFPNG_FN uint32_t cfpng_cost(uint32_t v)
{
	return v < 128u ? v : 256u - v;
}

// the lowest type among the smallest sums
CFPNG_FN uint32_t cfpng_choose(const uint64_t sums[CFPNG_FILTERS])
{
	uint32_t best = 0u;
	for (uint32_t t = 1u; t < CFPNG_FILTERS; ++t)
		if (sums[t] < sums[best])
			best = t;
	return best;
}

// ---- CRC-32 (IEEE, reflected: zlib.crc32) --------------------------------------------------------------------------
// The register without the initial and final inversion is linear over GF(2): reg(A || B) = reg(A) x^(8 |B|) + reg(B)
// modulo the polynomial.  A polynomial is a word with x^0 in bit 31 (zlib's crc32_combine writes them the same way).
#if defined(__HIPCC__)
#define CFPNG_CONSTEXPR __host__ __device__ constexpr
#else
#define CFPNG_CONSTEXPR constexpr
#endif

CFPNG_CONSTEXPR uint32_t cfpng_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0u;
	for (uint32_t i = 0; i < 32u; ++i) {
		p ^= b & (0u - ((a >> (31u - i)) & 1u));
		b = (b >> 1) ^ (CFPNG_POLY & (0u - (b & 1u)));
	}
	return p;
}

struct cfpng_tables {
	uint32_t sq[32];               // x^(2^k)
	uint32_t sub[CFPNG_SUBS];      // x^(8 CFPNG_SUB j): what moves a lane's register j lanes' bytes further from the end
};

CFPNG_CONSTEXPR cfpng_tables cfpng_make_tables()
{
	cfpng_tables t = {};
	t.sq[0] = 0x40000000u;
	for (uint32_t k = 1; k < 32u; ++k)
		t.sq[k] = cfpng_mulmod(t.sq[k - 1u], t.sq[k - 1u]);
	uint32_t step = 0x80000000u;
	for (uint32_t k = 0; k < 32u; ++k)
		if ((8u*CFPNG_SUB >> k) & 1u)
			step = cfpng_mulmod(step, t.sq[k]);
	t.sub[0] = 0x80000000u;
	for (uint32_t j = 1; j < CFPNG_SUBS; ++j)
		t.sub[j] = cfpng_mulmod(t.sub[j - 1u], step);
	return t;
}

// x^bits; x^(2^32) = x^1 modulo the polynomial, so the squares repeat with period 32
CFPNG_FN uint32_t cfpng_xpow(const uint32_t sq[32], uint64_t bits)
{
	uint32_t p = 0x80000000u;
	for (uint32_t k = 0; bits; bits >>= 1, ++k)
		if (bits & 1u)
			p = cfpng_mulmod(sq[k & 31u], p);
	return p;
}

// one entry of the byte table
CFPNG_CONSTEXPR uint32_t cfpng_crc_entry(uint32_t i)
{
	for (int k = 0; k < 8; ++k)
		i = (i >> 1) ^ (CFPNG_POLY & (0u - (i & 1u)));
	return i;
}

// the register after n more bytes
CFPNG_FN uint32_t cfpng_crc_bytes(const uint32_t table[256], uint32_t reg, const uint8_t* p, size_t n)
{
	for (size_t i = 0; i < n; ++i)
		reg = table[(reg ^ p[i]) & 255u] ^ (reg >> 8);
	return reg;
}

// the same without a table, for a few bytes: the chunk headers, a stream's last bytes
CFPNG_FN uint32_t cfpng_crc_few(uint32_t reg, const uint8_t* p, size_t n)
{
	for (size_t i = 0; i < n; ++i)
		reg = cfpng_crc_entry((reg ^ p[i]) & 255u) ^ (reg >> 8);
	return reg;
}

CFPNG_FN uint32_t cfpng_crc32_small(const uint8_t* p, size_t n)
{
	return ~cfpng_crc_few(0xFFFFFFFFu, p, n);
}

// The IDAT chunk's CRC from the parts the kernels make.  `full`: the XOR over the stream's whole CFPNG_SUB-byte pieces,
// counted from the stream's START, of register(piece) x^(8 CFPNG_SUB j), j pieces lying between it and the last whole
// one; `tail`: the len % CFPNG_SUB bytes behind them.
CFPNG_FN uint32_t cfpng_idat_crc(const uint32_t sq[32], uint32_t full, const uint8_t* tail, uint64_t len)
{
	const uint32_t r = (uint32_t)(len % CFPNG_SUB);
	const uint8_t type[4] = {'I', 'D', 'A', 'T'};
	const uint32_t head = cfpng_crc_few(0xFFFFFFFFu, type, 4);                // the register behind the chunk type
	uint32_t reg = cfpng_mulmod(head, cfpng_xpow(sq, 8u*len));
	reg ^= cfpng_mulmod(full, cfpng_xpow(sq, 8u*r));
	reg ^= cfpng_crc_few(0u, tail, r);
	return ~reg;
}

// ---- the bytes around the IDAT data --------------------------------------------------------------------------------
CFPNG_FN void cfpng_be32(uint8_t* p, uint32_t v)
{
	p[0] = (uint8_t)(v >> 24);
	p[1] = (uint8_t)(v >> 16);
	p[2] = (uint8_t)(v >> 8);
	p[3] = (uint8_t)v;
}

struct cfpng_head {
	uint32_t w[14];                // the file up to the IDAT data as little-endian words (a kernel argument), the IDAT
	                               // length still 0
	uint32_t bytes;                // 41 or 54: cfpng_data_offset
};

CFPNG_FN uint8_t cfpng_head_byte(const cfpng_head* h, uint32_t i)
{
	return (uint8_t)(h->w[i >> 2] >> (8u*(i & 3u)));
}

// signature, IHDR, sRGB (rendering intent 0) where asked for, and the IDAT chunk's length (0 for now) and type
CFPNG_FN void cfpng_write_head(cfpng_head* h, uint32_t width, uint32_t height, int color_type, int bit_depth, int srgb)
{
	static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
	uint8_t b[56];
	memset(b, 0, sizeof(b));
	uint8_t* p = b;
	memcpy(p, sig, 8);
	p += 8;
	cfpng_be32(p, 13u);
	memcpy(p + 4, "IHDR", 4);
	cfpng_be32(p + 8, width);
	cfpng_be32(p + 12, height);
	p[16] = (uint8_t)bit_depth;
	p[17] = (uint8_t)color_type;
	p[18] = p[19] = p[20] = 0u;     // compression 0, filter method 0, no interlace
	cfpng_be32(p + 21, cfpng_crc32_small(p + 4, 17));
	p += 25;
	if (srgb) {
		cfpng_be32(p, 1u);
		memcpy(p + 4, "sRGB", 4);
		p[8] = 0u;
		cfpng_be32(p + 9, cfpng_crc32_small(p + 4, 5));
		p += 13;
	}
	memcpy(p + 4, "IDAT", 4);
	h->bytes = (uint32_t)(p + 8 - b);
	for (uint32_t i = 0; i < 14u; ++i)
		h->w[i] = b[4u*i] | (uint32_t)b[4u*i + 1u] << 8 | (uint32_t)b[4u*i + 2u] << 16 | (uint32_t)b[4u*i + 3u] << 24;
}

// behind `len` bytes of IDAT data at file + data_offset: the chunk's length before them; its CRC and IEND behind them
CFPNG_FN void cfpng_write_tail(uint8_t* file, uint32_t data_offset, uint32_t len, uint32_t crc)
{
	static const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
	cfpng_be32(file + data_offset - 8u, len);
	uint8_t* p = file + data_offset + len;
	cfpng_be32(p, crc);
	for (uint32_t i = 0; i < 12u; ++i)
		p[4u + i] = iend[i];
}

#ifdef __HIPCC__
// ---- device side ---------------------------------------------------------------------------------------------------
struct cfpng_layout {
	size_t filtered, zstream, state, total;
};

// zstream_bytes: 0 where the stream is written in place
inline cfpng_layout cfpng_scratch(size_t filtered_bytes, size_t zstream_bytes)
{
	auto up = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
	cfpng_layout l;
	size_t o = 0;
	l.filtered = o; o = up(o + filtered_bytes);
	l.zstream = o;  o = up(o + zstream_bytes);
	l.state = o;    o = up(o + CFPNG_S_WORDS*4u);
	l.total = o;
	return l;
}

// The filtered bytes of an image (height x (1 + width x bpp)) into `filtered` (4-byte aligned) and the rows per filter
// type added to state[CFPNG_S_ROWS ..].  pixels: aligned to the texel, rows `pitch` bytes apart.
extern "C" hipError_t cfhip_launch_png_filter(const void* pixels, int pixel_type, size_t pitch, uint32_t width, uint32_t height,
	int color_type, int bit_depth, uint8_t* filtered, uint32_t* state, hipStream_t stream);

// The CRC shares of the zlib stream at `z` (4-byte aligned; its length is the deflate result's bytes_out in the state,
// at most zbound) into state[CFPNG_S_CRC]; dst != z: the stream is copied to dst as well (any alignment).
extern "C" hipError_t cfhip_launch_png_crc(const uint8_t* z, uint8_t* dst, uint64_t zbound, uint32_t* state, hipStream_t stream);

// Everything around the IDAT data into `file`, and the 15 words of cfhip_png_result at `result`.
extern "C" hipError_t cfhip_launch_png_final(const cfpng_head* head, const uint8_t* z, uint64_t filtered_bytes, const uint32_t* state,
	uint8_t* file, unsigned long long* result, hipStream_t stream);
#endif

#endif
