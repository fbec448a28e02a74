// The host part of the texel vocabulary (csrc/cf_texel.h) on the CPU, for tests/test_texel_host.py.  Raw little-endian
// arrays in and out, so that every bit pattern passes through unchanged:
//   texel_host decode              -> 256 floats (cf_u8_to_float of 0 ... 255), then 65536 (cf_half_to_float of every pattern)
//   texel_host unit_u8  < doubles  -> one byte each (cf_unit_to_u8)
//   texel_host to_half  < floats   -> one uint16 each (cf_float_to_half)
//   texel_host coords <side> ...   -> text: "size <type> <bytes>" per pixel type; per side and at in [-3 side, 3 side]
//                                     "<side> <at> <floor_mod> <there, unwrapped> <there, wrapped> <at, wrapped>";
//                                     and the same line for side 1 at INT32_MIN + 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cuttlefish_amd/csrc/cf_texel.h"

static_assert(cf_pixel_size(CFHIP_PIXEL_RGBA8) == 4u && cf_pixel_size(CFHIP_PIXEL_RGBA16F) == 8u &&
	cf_pixel_size(CFHIP_PIXEL_RGBA32F) == 16u, "constexpr");

template <class T>
static std::vector<T> read_all()
{
	std::vector<T> v;
	T buf[4096];
	size_t n;
	while ((n = fread(buf, sizeof(T), 4096, stdin)) > 0)
		v.insert(v.end(), buf, buf + n);
	return v;
}

template <class T>
static int write_all(const std::vector<T>& v)
{
	return fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size() ? 0 : 1;
}

static void coord_line(uint32_t side, int32_t at)
{
	int32_t plain = at, wrapped = at;
	const bool there = cf_wrap_coord(plain, side, false), there_w = cf_wrap_coord(wrapped, side, true);
	if (plain != at) {
		fprintf(stderr, "an unwrapped coordinate moved: %d -> %d\n", at, plain);
		exit(1);
	}
	printf("%u %d %d %d %d %d\n", side, at, cf_floor_mod(at, side), there ? 1 : 0, there_w ? 1 : 0, wrapped);
}

int main(int argc, char** argv)
{
	const char* mode = argc > 1 ? argv[1] : "";
	if (!strcmp(mode, "decode")) {
		std::vector<float> out;
		for (uint32_t v = 0; v < 256u; ++v)
			out.push_back(cf_u8_to_float(v));
		for (uint32_t h = 0; h < 65536u; ++h)
			out.push_back(cf_half_to_float(h));
		return write_all(out);
	}
	if (!strcmp(mode, "unit_u8")) {
		std::vector<uint8_t> out;
		for (double v : read_all<double>())
			out.push_back(cf_unit_to_u8(v));
		return write_all(out);
	}
	if (!strcmp(mode, "to_half")) {
		std::vector<uint16_t> out;
		for (float v : read_all<float>())
			out.push_back(cf_float_to_half(v));
		return write_all(out);
	}
	if (!strcmp(mode, "coords") && argc > 2) {
		for (int type : {CFHIP_PIXEL_RGBA8, CFHIP_PIXEL_RGBA32F, CFHIP_PIXEL_RGBA16F})
			printf("size %d %u\n", type, cf_pixel_size(type));
		for (int a = 2; a < argc; ++a) {
			const uint32_t side = (uint32_t)strtoul(argv[a], nullptr, 10);
			for (int32_t at = -3*(int32_t)side; at <= 3*(int32_t)side; ++at)
				coord_line(side, at);
		}
		coord_line(1u, INT32_MIN + 1);
		return 0;
	}
	fprintf(stderr, "usage: %s decode | unit_u8 | to_half | coords <side> ...\n", argv[0]);
	return 2;
}
