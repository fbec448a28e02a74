// png.hip -- PNG files of images on gfx950.  THE DEFINITION of every byte written is
// tests/png_ref.py; these kernels and the zlib encoder between them (deflate.hip) return it exactly.
//
//   filter   one workgroup of four wavefronts per row, or per four rows of at most 256 pixels.  A wavefront walks its
//            part of the row 64 pixels at a time.  Pass 1 forms the raw bytes of the row and of the row above from the
//            source texels -- quantised, channel-selected, 16-bit samples swapped -- and adds up the cost of the five
//            filters; the pixel to the left comes from the lane before (the first lane's from the trip before), so
//            every texel is loaded once per pass.  The sums are reduced, the lowest type among the smallest wins.  Pass
//            2 forms the bytes again (the texels now hit L2), filters them with the chosen type into LDS at the output's
//            own alignment and writes them out as whole words, single bytes at the two ends.  No intermediate image.
//   deflate  cfhip_deflate's eight stages on the filtered bytes
//   crc      one workgroup per 16 KiB of the zlib stream, whose length only the device knows: a lane takes the
//            register of 64 bytes from a byte table in LDS, moves it to the end of the workgroup's piece with one
//            multiplication by x^(512 j) modulo the polynomial (a table made at compile time), the workgroup XORs its
//            lanes, one lane moves the piece to the end of the last whole 64 bytes by square and multiply and XORs it
//            into one word.  XOR does not depend on the order.  The same kernel copies the stream behind the IDAT header
//            where the encoder could not write it there
//   final    the signature, IHDR, sRGB, the IDAT length, the IDAT CRC (the chunk type in front, the last len % 64 bytes
//            behind), IEND and the result, by one lane in plain C++
#include "cf_texel.h"
#include "png.h"

namespace {

__device__ const cfpng_tables kTab = cfpng_make_tables();

template <int PIX>
__device__ __forceinline__ void png_load(const uint8_t* p, uint32_t w[4])
{
	w[1] = w[2] = w[3] = 0u;
	if (PIX == CFPNG_PIX_RGBA8)
		w[0] = *reinterpret_cast<const uint32_t*>(p);
	else if (PIX == CFPNG_PIX_RGBA16F) {
		const uint2 v = *reinterpret_cast<const uint2*>(p);
		w[0] = v.x; w[1] = v.y;
	} else {
		const uint4 v = *reinterpret_cast<const uint4*>(p);
		w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
	}
}

// a pixel's bytes from the lane before / from one given lane: only the words the pixel has
template <int BPP>
__device__ __forceinline__ uint64_t png_shfl_up1(uint64_t v)
{
	uint64_t r = (uint32_t)__shfl_up((uint32_t)v, 1, 64);
	if (BPP > 4)
		r |= (uint64_t)(uint32_t)__shfl_up((uint32_t)(v >> 32), 1, 64) << 32;
	return r;
}

template <int BPP>
__device__ __forceinline__ uint64_t png_shfl_from(uint64_t v, int lane)
{
	uint64_t r = (uint32_t)__shfl((uint32_t)v, lane, 64);
	if (BPP > 4)
		r |= (uint64_t)(uint32_t)__shfl((uint32_t)(v >> 32), lane, 64) << 32;
	return r;
}

__device__ __forceinline__ uint32_t png_byte(uint64_t px, uint32_t k)
{
	return (uint32_t)(px >> (8u*k)) & 255u;
}

// One wavefront's view of its part [x0, x1) of row y: trip t gives every lane its pixel and the three around it.
template <int PIX, int CH, int D16>
struct PngRow {
	static constexpr uint32_t BPP = CH*(D16 ? 2 : 1);
	const uint8_t* cur;            // the row's texels
	const uint8_t* up;             // the row above's, NULL for the first row
	uint32_t x0, x1, lane;
	uint64_t carry_c, carry_u;     // the pixel left of the trip's first one, in this row and above

	__device__ __forceinline__ uint64_t pixel(const uint8_t* row, uint32_t x) const
	{
		uint32_t w[4];
		png_load<PIX>(row + (size_t)x*cf_pixel_size(PIX), w);
		return cfpng_pixel<PIX, CH, D16>(w);
	}

	__device__ __forceinline__ void start(bool need_up)
	{
		carry_c = carry_u = 0u;
		if (x0 > 0u && x0 < x1) {                              // wave-uniform: the pixel before the part
			carry_c = pixel(cur, x0 - 1u);
			if (up && need_up)
				carry_u = pixel(up, x0 - 1u);
		}
	}

	// -> whether this lane has a pixel in trip t; pc: it, pu: above, lc: left, lu: above left
	__device__ __forceinline__ bool trip(uint32_t t, bool need_up, uint64_t& pc, uint64_t& pu, uint64_t& lc, uint64_t& lu)
	{
		const uint32_t x = x0 + t*64u + lane;
		const bool act = x < x1;
		pc = pu = 0u;
		if (act) {
			pc = pixel(cur, x);
			if (up && need_up)
				pu = pixel(up, x);
		}
		lc = png_shfl_up1<BPP>(pc);
		lu = png_shfl_up1<BPP>(pu);
		if (lane == 0u) {
			lc = carry_c;
			lu = carry_u;
		}
		carry_c = png_shfl_from<BPP>(pc, 63);
		carry_u = png_shfl_from<BPP>(pu, 63);
		return act;
	}
};

template <int PIX, int CH, int D16>
__global__ __launch_bounds__(256) void cfhip_png_filter_kernel(const uint8_t* __restrict__ pixels, size_t pitch, uint32_t width,
	uint32_t height, uint32_t waves_per_row, uint8_t* __restrict__ filtered, uint32_t* __restrict__ state)
{
	constexpr uint32_t BPP = CH*(D16 ? 2 : 1);
	__shared__ uint32_t s_stage[4][132];               // per wavefront: 64 pixels of 8 bytes and 3 bytes of alignment
	__shared__ unsigned long long s_sum[4][CFPNG_FILTERS];
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	const uint32_t whole = waves_per_row == 4u;        // the workgroup takes one row; otherwise a wavefront does
	const uint32_t y = whole ? blockIdx.x : blockIdx.x*4u + wave;
	const bool live = y < height;
	const uint32_t seg = whole ? (width + 3u)/4u : width;
	const uint32_t trips = (seg + 63u)/64u;            // the same for every wavefront: the barriers below are uniform
	const uint32_t part = whole ? wave : 0u;
	const uint32_t rb = width*BPP;

	PngRow<PIX, CH, D16> row;
	row.lane = lane;
	row.x0 = live ? (part*seg < width ? part*seg : width) : 0u;
	row.x1 = live ? (width - row.x0 < seg ? width : row.x0 + seg) : 0u;
	row.cur = pixels + (size_t)(live ? y : 0u)*pitch;
	row.up = live && y > 0u ? row.cur - pitch : nullptr;

	// pass 1: the five sums
	uint32_t sum[CFPNG_FILTERS] = {0u, 0u, 0u, 0u, 0u};
	row.start(true);
	for (uint32_t t = 0; t < trips; ++t) {
		uint64_t pc, pu, lc, lu;
		if (row.trip(t, true, pc, pu, lc, lu)) {
#pragma unroll
			for (uint32_t k = 0; k < BPP; ++k) {
				const uint32_t x = png_byte(pc, k), a = png_byte(lc, k), b = png_byte(pu, k), c = png_byte(lu, k);
				sum[0] += cfpng_cost(x);
				sum[1] += cfpng_cost((x - a) & 255u);
				sum[2] += cfpng_cost((x - b) & 255u);
				sum[3] += cfpng_cost((x - ((a + b) >> 1)) & 255u);
				sum[4] += cfpng_cost((x - cfpng_paeth(a, b, c)) & 255u);
			}
		}
	}
	// a lane's sum stays below 2^32 for any row this writer takes (fewer than 2^31 bytes); a row's need not
	uint64_t total[CFPNG_FILTERS];
#pragma unroll
	for (uint32_t f = 0; f < CFPNG_FILTERS; ++f) {
		unsigned long long v = sum[f];
		for (int s = 32; s; s >>= 1)
			v += __shfl_xor(v, s, 64);
		total[f] = v;
	}
	if (whole) {
		if (lane == 0u)
			for (uint32_t f = 0; f < CFPNG_FILTERS; ++f)
				s_sum[wave][f] = total[f];
		__syncthreads();
#pragma unroll
		for (uint32_t f = 0; f < CFPNG_FILTERS; ++f)
			total[f] = s_sum[0][f] + s_sum[1][f] + s_sum[2][f] + s_sum[3][f];
	}
	const uint32_t type = cfpng_choose(total);
	const uint32_t row_at = y*(1u + rb);               // below 2^31
	if (live && lane == 0u && part == 0u) {
		filtered[row_at] = (uint8_t)type;
		atomicAdd(&state[CFPNG_S_ROWS + type], 1u);
	}

	// pass 2: the chosen filter's bytes
	const bool need_up = type >= 2u;
	uint8_t* sb = reinterpret_cast<uint8_t*>(s_stage[wave]);
	row.start(need_up);
	for (uint32_t t = 0; t < trips; ++t) {
		uint64_t pc, pu, lc, lu;
		const bool act = row.trip(t, need_up, pc, pu, lc, lu);
		const uint32_t xb = row.x0 + t*64u;                                    // the trip's first pixel
		const uint32_t npix = xb < row.x1 ? (row.x1 - xb < 64u ? row.x1 - xb : 64u) : 0u;
		const uint32_t g0 = row_at + 1u + xb*BPP, gend = g0 + npix*BPP;        // the trip's bytes in `filtered`
		const uint32_t sh = g0 & 3u;
		if (act) {
#pragma unroll
			for (uint32_t k = 0; k < BPP; ++k)
				sb[sh + lane*BPP + k] = (uint8_t)cfpng_filter(type, png_byte(pc, k), png_byte(lc, k), png_byte(pu, k),
					png_byte(lu, k));
		}
		__syncthreads();
		if (npix) {
			const uint32_t al = (g0 + 3u) & ~3u;
			const uint32_t gw0 = al < gend ? al : gend;                        // whole words lie in [gw0, gw1)
			const uint32_t gw1 = (gend & ~3u) > gw0 ? (gend & ~3u) : gw0;
			const uint32_t head = gw0 - g0, words = (gw1 - gw0) >> 2, tail = gend - gw1;
			if (lane < head)
				filtered[g0 + lane] = sb[sh + lane];
			uint32_t* gout = reinterpret_cast<uint32_t*>(filtered + gw0);
			const uint32_t* sw = s_stage[wave] + ((sh + head) >> 2);
			for (uint32_t i = lane; i < words; i += 64u)
				gout[i] = sw[i];
			if (lane < tail)
				filtered[gw1 + lane] = sb[sh + (gw1 - g0) + lane];
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(256) void cfhip_png_crc_kernel(const uint8_t* z, uint8_t* dst,
	uint32_t* __restrict__ state)
{
	__shared__ uint32_t s_table[256];
	__shared__ uint32_t s_red[4];
	const uint32_t tid = threadIdx.x;
	const unsigned long long len = reinterpret_cast<const unsigned long long*>(state + CFPNG_S_DEFLATE)[1];
	const unsigned long long nfull = len/CFPNG_SUB;
	const unsigned long long j0 = (unsigned long long)blockIdx.x*CFPNG_SUBS;    // pieces counted from the last whole one
	const bool copy = dst != z;
	if (blockIdx.x == 0u && copy)
		for (unsigned long long i = nfull*CFPNG_SUB + tid; i < len; i += 256u)
			dst[i] = z[i];
	if (j0 >= nfull)
		return;
	s_table[tid] = cfpng_crc_entry(tid);
	__syncthreads();
	const uint32_t cnt = nfull - j0 < CFPNG_SUBS ? (uint32_t)(nfull - j0) : CFPNG_SUBS;
	const unsigned long long lo = (nfull - j0 - cnt)*CFPNG_SUB;                  // the workgroup's bytes: [lo, lo + 64 cnt)
	if (copy) {
		const uint32_t* zw = reinterpret_cast<const uint32_t*>(z + lo);
		uint8_t* d = dst + lo;
		for (uint32_t i = tid; i < cnt*(CFPNG_SUB/4u); i += 256u) {
			const uint32_t w = zw[i];
			d[4u*i] = (uint8_t)w;
			d[4u*i + 1u] = (uint8_t)(w >> 8);
			d[4u*i + 2u] = (uint8_t)(w >> 16);
			d[4u*i + 3u] = (uint8_t)(w >> 24);
		}
	}
	uint32_t share = 0u;
	if (tid < cnt) {
		// lane tid takes the piece that lies tid pieces before the workgroup's last
		const uint32_t* p = reinterpret_cast<const uint32_t*>(z + lo + (size_t)(cnt - 1u - tid)*CFPNG_SUB);
		uint32_t reg = 0u;
#pragma unroll 4
		for (uint32_t i = 0; i < CFPNG_SUB/4u; ++i) {
			reg ^= p[i];
			reg = s_table[reg & 255u] ^ (reg >> 8);
			reg = s_table[reg & 255u] ^ (reg >> 8);
			reg = s_table[reg & 255u] ^ (reg >> 8);
			reg = s_table[reg & 255u] ^ (reg >> 8);
		}
		share = cfpng_mulmod(reg, kTab.sub[tid]);
	}
	for (int s = 32; s; s >>= 1)
		share ^= __shfl_xor(share, s, 64);
	if ((tid & 63u) == 0u)
		s_red[tid >> 6] = share;
	__syncthreads();
	if (tid == 0u) {
		const uint32_t piece = s_red[0] ^ s_red[1] ^ s_red[2] ^ s_red[3];
		atomicXor(&state[CFPNG_S_CRC], cfpng_mulmod(piece, cfpng_xpow(kTab.sq, 8ull*CFPNG_SUB*j0)));
	}
}

__global__ void cfhip_png_final_kernel(cfpng_head head, const uint8_t* __restrict__ z, unsigned long long filtered_bytes,
	const uint32_t* __restrict__ state, uint8_t* __restrict__ file, unsigned long long* __restrict__ result)
{
	if (threadIdx.x || blockIdx.x)
		return;
	const unsigned long long* df = reinterpret_cast<const unsigned long long*>(state + CFPNG_S_DEFLATE);
	const unsigned long long len = df[1];
#pragma unroll
	for (uint32_t i = 0; i < sizeof(head.w)/4u; ++i)
#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k)
			if (4u*i + k < head.bytes)
				file[4u*i + k] = (uint8_t)(head.w[i] >> (8u*k));
	const uint32_t crc = cfpng_idat_crc(kTab.sq, state[CFPNG_S_CRC], z + len/CFPNG_SUB*CFPNG_SUB, len);
	cfpng_write_tail(file, head.bytes, (uint32_t)len, crc);
	result[0] = head.bytes + len + CFPNG_TAIL;
	result[1] = len;
	result[2] = filtered_bytes;
	result[3] = state[CFPNG_S_ROWS] | (unsigned long long)state[CFPNG_S_ROWS + 1] << 32;
	result[4] = state[CFPNG_S_ROWS + 2] | (unsigned long long)state[CFPNG_S_ROWS + 3] << 32;
	result[5] = state[CFPNG_S_ROWS + 4] | (unsigned long long)crc << 32;
	for (uint32_t i = 0; i < 9u; ++i)
		result[6u + i] = df[i];
}

template <int PIX, int CH>
hipError_t png_filter_depth(int bit_depth, dim3 grid, hipStream_t stream, const uint8_t* pixels, size_t pitch, uint32_t width,
	uint32_t height, uint32_t waves_per_row, uint8_t* filtered, uint32_t* state)
{
	if (bit_depth == 16)
		hipLaunchKernelGGL((cfhip_png_filter_kernel<PIX, CH, 1>), grid, dim3(256), 0, stream, pixels, pitch, width, height,
			waves_per_row, filtered, state);
	else
		hipLaunchKernelGGL((cfhip_png_filter_kernel<PIX, CH, 0>), grid, dim3(256), 0, stream, pixels, pitch, width, height,
			waves_per_row, filtered, state);
	return hipGetLastError();
}

template <int PIX>
hipError_t png_filter_channels(uint32_t channels, int bit_depth, dim3 grid, hipStream_t stream, const uint8_t* pixels, size_t pitch,
	uint32_t width, uint32_t height, uint32_t waves_per_row, uint8_t* filtered, uint32_t* state)
{
	switch (channels) {
		case 1: return png_filter_depth<PIX, 1>(bit_depth, grid, stream, pixels, pitch, width, height, waves_per_row, filtered, state);
		case 2: return png_filter_depth<PIX, 2>(bit_depth, grid, stream, pixels, pitch, width, height, waves_per_row, filtered, state);
		case 3: return png_filter_depth<PIX, 3>(bit_depth, grid, stream, pixels, pitch, width, height, waves_per_row, filtered, state);
		case 4: return png_filter_depth<PIX, 4>(bit_depth, grid, stream, pixels, pitch, width, height, waves_per_row, filtered, state);
		default: return hipErrorInvalidValue;
	}
}

} // namespace

extern "C" hipError_t cfhip_launch_png_filter(const void* pixels, int pixel_type, size_t pitch, uint32_t width, uint32_t height,
	int color_type, int bit_depth, uint8_t* filtered, uint32_t* state, hipStream_t stream)
{
	const uint32_t channels = cfpng_channels(color_type);
	// a row of at most 256 pixels is a wavefront's (four trips); a longer one is split over the workgroup's four
	const uint32_t waves_per_row = width > 256u ? 4u : 1u;
	const dim3 grid(waves_per_row == 4u ? height : (height + 3u)/4u);
	const uint8_t* p = static_cast<const uint8_t*>(pixels);
	switch (pixel_type) {
		case CFPNG_PIX_RGBA8:
			return png_filter_channels<CFPNG_PIX_RGBA8>(channels, bit_depth, grid, stream, p, pitch, width, height, waves_per_row, filtered, state);
		case CFPNG_PIX_RGBA32F:
			return png_filter_channels<CFPNG_PIX_RGBA32F>(channels, bit_depth, grid, stream, p, pitch, width, height, waves_per_row, filtered, state);
		case CFPNG_PIX_RGBA16F:
			return png_filter_channels<CFPNG_PIX_RGBA16F>(channels, bit_depth, grid, stream, p, pitch, width, height, waves_per_row, filtered, state);
		default:
			return hipErrorInvalidValue;
	}
}

extern "C" hipError_t cfhip_launch_png_crc(const uint8_t* z, uint8_t* dst, uint64_t zbound, uint32_t* state, hipStream_t stream)
{
	const uint64_t pieces = zbound/CFPNG_SUB;
	const uint64_t blocks = (pieces + CFPNG_SUBS - 1u)/CFPNG_SUBS;
	hipLaunchKernelGGL(cfhip_png_crc_kernel, dim3((uint32_t)(blocks ? blocks : 1u)), dim3(256), 0, stream, z, dst, state);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_png_final(const cfpng_head* head, const uint8_t* z, uint64_t filtered_bytes, const uint32_t* state,
	uint8_t* file, unsigned long long* result, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_png_final_kernel, dim3(1), dim3(64), 0, stream, *head, z, (unsigned long long)filtered_bytes, state, file,
		result);
	return hipGetLastError();
}
