// png_host.cpp -- the PNG writer's shared logic (csrc/png.h) on the CPU, with the host compiler alone: the exact functions
// the kernels of csrc/png.hip call for a pixel's bytes, the five filters and their cost, the choice, the bytes around
// the IDAT data, and the CRC of pieces combined by multiplication modulo the polynomial.  tests/test_png_host.py compares
// it with the definition, tests/png_ref.py; a build with -fsanitize=address,undefined checks the same logic for reads and
// writes out of range (every buffer is a heap block of its exact size).
//
//   c++ -std=c++17 -O1 -o png_host tools/png_host.cpp -lz
//   png_host encode image.bin out.png      image.bin: seven uint32 (little endian) width, height, pixel type, pitch in
//                                          bytes, colour type, bit depth, sRGB, then height x pitch bytes of texels.
//                                          The IDAT body is a zlib stream of STORED blocks of the filtered bytes.
//                                          Prints: rows per filter type (5), the IDAT CRC, the filtered bytes' CRC-32
//   png_host read file.png out.raw         checks every chunk (the IDAT CRC both ways: byte by byte, and from pieces as
//                                          the kernels take it), inflates with zlib, undoes the filters, writes the raw
//                                          rows.  Prints: width height depth colour-type sRGB, then the rows' types
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include <zlib.h>

#include "../cuttlefish_amd/csrc/png.h"

static const cfpng_tables kTab = cfpng_make_tables();

static std::vector<uint8_t> slurp(const char* path)
{
	std::vector<uint8_t> v;
	FILE* f = fopen(path, "rb");
	if (!f) {
		perror(path);
		exit(2);
	}
	uint8_t buf[65536];
	size_t n;
	while ((n = fread(buf, 1, sizeof(buf), f)) > 0)
		v.insert(v.end(), buf, buf + n);
	fclose(f);
	return v;
}

static uint32_t le32(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint32_t be32(const uint8_t* p) { return p[3] | (uint32_t)p[2] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[0] << 24; }

// The IDAT chunk's CRC the way the crc and final kernels take it: a register per whole 64 bytes, moved to the end of its
// piece of 256 by the table, the piece moved to the end of the last whole 64 bytes by square and multiply, all XORed.
static uint32_t idat_crc_from_pieces(const uint8_t* z, uint64_t len)
{
	uint32_t table[256];
	for (uint32_t i = 0; i < 256u; ++i)
		table[i] = cfpng_crc_entry(i);
	const uint64_t nfull = len/CFPNG_SUB;
	uint32_t full = 0u;
	for (uint64_t j0 = 0; j0 < nfull; j0 += CFPNG_SUBS) {
		const uint32_t cnt = nfull - j0 < CFPNG_SUBS ? (uint32_t)(nfull - j0) : CFPNG_SUBS;
		const uint64_t lo = (nfull - j0 - cnt)*CFPNG_SUB;
		uint32_t piece = 0u;
		for (uint32_t t = 0; t < cnt; ++t)
			piece ^= cfpng_mulmod(cfpng_crc_bytes(table, 0u, z + lo + (size_t)(cnt - 1u - t)*CFPNG_SUB, CFPNG_SUB), kTab.sub[t]);
		full ^= cfpng_mulmod(piece, cfpng_xpow(kTab.sq, 8ull*CFPNG_SUB*j0));
	}
	return cfpng_idat_crc(kTab.sq, full, z + nfull*CFPNG_SUB, len);
}

template <int PIX, int CH, int D16>
static uint64_t pixel_at(const uint8_t* texel)
{
	uint32_t w[4] = {0u, 0u, 0u, 0u};
	memcpy(w, texel, PIX == CFPNG_PIX_RGBA8 ? 4 : PIX == CFPNG_PIX_RGBA16F ? 8 : 16);
	return cfpng_pixel<PIX, CH, D16>(w);
}

typedef uint64_t (*pixel_fn)(const uint8_t*);

template <int PIX, int CH>
static pixel_fn pick_depth(int depth) { return depth == 16 ? pixel_at<PIX, CH, 1> : pixel_at<PIX, CH, 0>; }

template <int PIX>
static pixel_fn pick_channels(uint32_t ch, int depth)
{
	return ch == 1 ? pick_depth<PIX, 1>(depth) : ch == 2 ? pick_depth<PIX, 2>(depth) : ch == 3 ? pick_depth<PIX, 3>(depth) :
		pick_depth<PIX, 4>(depth);
}

static int encode(const char* in_path, const char* out_path)
{
	const std::vector<uint8_t> in = slurp(in_path);
	if (in.size() < 28) {
		fprintf(stderr, "short image file\n");
		return 2;
	}
	const uint32_t width = le32(&in[0]), height = le32(&in[4]), pix = le32(&in[8]), pitch = le32(&in[12]);
	const int ct = (int)le32(&in[16]), depth = (int)le32(&in[20]), srgb = (int)le32(&in[24]);
	const uint32_t bpp = cfpng_bpp(ct, depth), tb = pix == CFPNG_PIX_RGBA8 ? 4u : pix == CFPNG_PIX_RGBA16F ? 8u : 16u;
	if (!bpp || !width || !height || pix > 2u || pitch < width*tb || in.size() != 28u + (size_t)height*pitch ||
		cfpng_filtered_bytes(width, height, bpp) >= (1u << 28)) {
		fprintf(stderr, "bad image file\n");
		return 2;
	}
	// the texels in a heap block of their exact size
	std::unique_ptr<uint8_t[]> texels(new uint8_t[(size_t)height*pitch]);
	memcpy(texels.get(), &in[28], (size_t)height*pitch);
	const pixel_fn px = pix == CFPNG_PIX_RGBA8 ? pick_channels<CFPNG_PIX_RGBA8>(cfpng_channels(ct), depth) :
		pix == CFPNG_PIX_RGBA16F ? pick_channels<CFPNG_PIX_RGBA16F>(cfpng_channels(ct), depth) :
		pick_channels<CFPNG_PIX_RGBA32F>(cfpng_channels(ct), depth);
	const size_t rb = (size_t)width*bpp, n = (size_t)cfpng_filtered_bytes(width, height, bpp);
	std::unique_ptr<uint8_t[]> filtered(new uint8_t[n]);
	uint32_t rows[CFPNG_FILTERS] = {0u, 0u, 0u, 0u, 0u};
	for (uint32_t y = 0; y < height; ++y) {
		const uint8_t* cur = texels.get() + (size_t)y*pitch;
		const uint8_t* up = y ? cur - pitch : nullptr;
		uint32_t type = 0u;
		for (int pass = 0; pass < 2; ++pass) {
			uint64_t sums[CFPNG_FILTERS] = {0u, 0u, 0u, 0u, 0u};
			uint64_t lc = 0u, lu = 0u;
			for (uint32_t x = 0; x < width; ++x) {
				const uint64_t pc = px(cur + (size_t)x*tb), pu = up ? px(up + (size_t)x*tb) : 0u;
				for (uint32_t k = 0; k < bpp; ++k) {
					const uint32_t v = (uint32_t)(pc >> (8u*k)) & 255u, a = (uint32_t)(lc >> (8u*k)) & 255u;
					const uint32_t b = (uint32_t)(pu >> (8u*k)) & 255u, c = (uint32_t)(lu >> (8u*k)) & 255u;
					if (pass == 0)
						for (uint32_t t = 0; t < CFPNG_FILTERS; ++t)
							sums[t] += cfpng_cost(cfpng_filter(t, v, a, b, c));
					else
						filtered[(size_t)y*(1u + rb) + 1u + (size_t)x*bpp + k] = (uint8_t)cfpng_filter(type, v, a, b, c);
				}
				lc = pc;
				lu = pu;
			}
			if (pass == 0) {
				type = cfpng_choose(sums);
				filtered[(size_t)y*(1u + rb)] = (uint8_t)type;
				++rows[type];
			}
		}
	}
	// a zlib stream of stored blocks
	std::vector<uint8_t> z = {0x78, 0x01};
	for (size_t at = 0; at < n || at == 0; at += 65535u) {
		const size_t len = n - at < 65535u ? n - at : 65535u;
		z.push_back(at + len >= n ? 1u : 0u);
		z.push_back((uint8_t)len);
		z.push_back((uint8_t)(len >> 8));
		z.push_back((uint8_t)~len);
		z.push_back((uint8_t)(~len >> 8));
		z.insert(z.end(), filtered.get() + at, filtered.get() + at + len);
		if (at + len >= n)
			break;
	}
	uint32_t a = 1u, b = 0u;
	for (size_t i = 0; i < n; ++i) {
		a = (a + filtered[i]) % 65521u;
		b = (b + a) % 65521u;
	}
	const uint32_t adler = b << 16 | a;
	for (int s = 24; s >= 0; s -= 8)
		z.push_back((uint8_t)(adler >> s));
	cfpng_head head;
	cfpng_write_head(&head, width, height, ct, depth, srgb);
	if (head.bytes != cfpng_data_offset(srgb) || head.bytes + z.size() + CFPNG_TAIL > cfpng_bound(width, height, ct, depth, srgb)) {
		fprintf(stderr, "the head or the bound is off\n");
		return 1;
	}
	const size_t total = head.bytes + z.size() + CFPNG_TAIL;
	std::unique_ptr<uint8_t[]> file(new uint8_t[total]);
	for (uint32_t i = 0; i < head.bytes; ++i)
		file[i] = cfpng_head_byte(&head, i);
	memcpy(file.get() + head.bytes, z.data(), z.size());
	const uint32_t crc = idat_crc_from_pieces(z.data(), z.size());
	cfpng_write_tail(file.get(), head.bytes, (uint32_t)z.size(), crc);
	FILE* f = fopen(out_path, "wb");
	if (!f || fwrite(file.get(), 1, total, f) != total) {
		perror(out_path);
		return 2;
	}
	fclose(f);
	printf("%u %u %u %u %u %u %lu\n", rows[0], rows[1], rows[2], rows[3], rows[4], crc, crc32(0L, filtered.get(), (uInt)n));
	return 0;
}

static int read_png(const char* in_path, const char* out_path)
{
	const std::vector<uint8_t> in = slurp(in_path);
	// the file in a heap block of its exact size
	std::unique_ptr<uint8_t[]> file(new uint8_t[in.size() ? in.size() : 1]);
	memcpy(file.get(), in.data(), in.size());
	const uint8_t* p = file.get();
	const size_t size = in.size();
	cfpng_head sig;
	cfpng_write_head(&sig, 1, 1, 0, 8, 0);
	if (size < 8)
		return 1;
	for (uint32_t i = 0; i < 8u; ++i)
		if (p[i] != cfpng_head_byte(&sig, i)) {
			fprintf(stderr, "not a PNG signature\n");
			return 1;
		}
	uint32_t table[256];
	for (uint32_t i = 0; i < 256u; ++i)
		table[i] = cfpng_crc_entry(i);
	uint32_t width = 0, height = 0, depth = 0, ct = 0, srgb = 0;
	const uint8_t* idat = nullptr;
	size_t idat_len = 0, at = 8;
	bool end = false;
	while (at < size) {
		if (size - at < 12 || be32(p + at) > size - at - 12) {
			fprintf(stderr, "a chunk leaves the file\n");
			return 1;
		}
		const uint32_t len = be32(p + at);
		const uint8_t* kind = p + at + 4;
		const uint32_t crc = be32(p + at + 8 + len);
		if (~cfpng_crc_bytes(table, 0xFFFFFFFFu, kind, 4u + (size_t)len) != crc || crc != crc32(0L, kind, 4u + len)) {
			fprintf(stderr, "chunk CRC\n");
			return 1;
		}
		if (!memcmp(kind, "IHDR", 4) && len == 13) {
			width = be32(kind + 4);
			height = be32(kind + 8);
			depth = kind[12];
			ct = kind[13];
			if (kind[14] || kind[15] || kind[16])
				return 1;
			// the head this writer makes is the one in the file
			cfpng_head h;
			cfpng_write_head(&h, width, height, (int)ct, (int)depth, 0);
			for (uint32_t i = 0; i < 33u; ++i)
				if (p[i] != cfpng_head_byte(&h, i)) {
					fprintf(stderr, "IHDR differs from cfpng_write_head\n");
					return 1;
				}
		} else if (!memcmp(kind, "sRGB", 4) && len == 1)
			srgb = 1;
		else if (!memcmp(kind, "IDAT", 4) && !idat) {
			idat = kind + 4;
			idat_len = len;
			if (idat_crc_from_pieces(idat, idat_len) != crc) {
				fprintf(stderr, "the CRC from pieces differs\n");
				return 1;
			}
		} else if (!memcmp(kind, "IEND", 4) && len == 0)
			end = true;
		else {
			fprintf(stderr, "unexpected chunk\n");
			return 1;
		}
		at += 12u + (size_t)len;
	}
	const uint32_t bpp = cfpng_bpp((int)ct, (int)depth);
	if (!end || !idat || !bpp || !width || !height || cfpng_filtered_bytes(width, height, bpp) >= (1u << 28))
		return 1;
	const size_t rb = (size_t)width*bpp, n = (size_t)cfpng_filtered_bytes(width, height, bpp);
	std::unique_ptr<uint8_t[]> raw(new uint8_t[n]);
	uLongf got = (uLongf)n;
	if (uncompress(raw.get(), &got, idat, (uLong)idat_len) != Z_OK || got != n) {
		fprintf(stderr, "the IDAT data does not inflate to the filtered size\n");
		return 1;
	}
	std::unique_ptr<uint8_t[]> rows(new uint8_t[rb*height]);
	printf("%u %u %u %u %u", width, height, depth, ct, srgb);
	for (uint32_t y = 0; y < height; ++y) {
		const uint32_t type = raw[(size_t)y*(1u + rb)];
		if (type >= CFPNG_FILTERS)
			return 1;
		printf(" %u", type);
		uint8_t* cur = rows.get() + (size_t)y*rb;
		for (size_t i = 0; i < rb; ++i) {
			const uint32_t a = i >= bpp ? cur[i - bpp] : 0u, b = y ? cur[i - rb] : 0u, c = (y && i >= bpp) ? cur[i - rb - bpp] : 0u;
			const uint32_t f = raw[(size_t)y*(1u + rb) + 1u + i];
			// filtered = x - pred: what cfpng_filter takes away from 0 is the prediction
			cur[i] = (uint8_t)(f - cfpng_filter(type, 0u, a, b, c));
		}
	}
	printf("\n");
	FILE* f = fopen(out_path, "wb");
	if (!f || fwrite(rows.get(), 1, rb*height, f) != rb*height) {
		perror(out_path);
		return 2;
	}
	fclose(f);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc == 4 && !strcmp(argv[1], "encode"))
		return encode(argv[2], argv[3]);
	if (argc == 4 && !strcmp(argv[1], "read"))
		return read_png(argv[2], argv[3]);
	fprintf(stderr, "usage: png_host encode image.bin out.png | png_host read file.png out.raw\n");
	return 2;
}
