// lzsize.hip -- the deflate-size estimate of a byte stream on gfx950.  THE DEFINITION is
// tests/lzsize_ref.py; these kernels return its numbers exactly, every one of them an integer sum.
//
// One slice (lzsize.h) runs five stages on one stream:
//   keys    one thread per position: (little-endian word at p, p)
//   sort    rocprim's stable radix sort of the pairs by key: equal keys then lie in ascending position, so the K entries
//           before an entry are its candidates, nearest first, and the first one outside the window ends the walk
//   match   one thread per sorted entry: word-wise common prefix against up to K candidates -> (L, D - 1) at p
//   parse   one wavefront per chunk of 4096 bytes: L / D staged in LDS, the lazy rule applied by all lanes, then ONE
//           LANE WALKS the chunk (p += L or 1: one dependent LDS read per token) and flags what it visits; all lanes
//           histogram the flagged positions in LDS and add the non-zero counters to the cost block's
//   cost    one wavefront per cost block: lg16 over the 316 counters, one 64-bit atomic add per sum
// The walk is the serial part: at most 4096 steps of one LDS round trip.  Pointer jumping would take 12 rounds over
// two more 8 KiB arrays per wavefront (five wavefronts per CU for nine) to shorten a chain that the other chunks
// in flight on the CU overlap.  That is an argument from the structure: DESIGN.md section 4.15 says what was measured.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "lzsize.h"

namespace {

__device__ __forceinline__ uint32_t lz_load32(const uint8_t* p)
{
	uint32_t v;
	__builtin_memcpy(&v, p, 4);
	return v;
}

// M = carry + n positions.  The first M - 3 have a key; the others (targets all, M >= 4 or not) get L = 0.
__global__ __launch_bounds__(256) void cfhip_lz_keys_kernel(const uint8_t* __restrict__ bytes, uint32_t m, uint32_t carry,
	uint32_t* __restrict__ keys, uint32_t* __restrict__ pos, uint32_t* __restrict__ ld)
{
	const uint32_t i = blockIdx.x*256u + threadIdx.x;
	if (i >= m)
		return;
	if (i + 3u < m) {
		// the two aligned words around i (the array is 256-byte aligned and padded by 16 bytes)
		const uint32_t* w = reinterpret_cast<const uint32_t*>(bytes) + (i >> 2);
		const unsigned long long both = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
		keys[i] = (uint32_t)(both >> (8u*(i & 3u)));
		pos[i] = i;
	} else if (i >= carry)
		ld[i - carry] = 0u;
}

// pairs = M - 3 sorted entries.  Entry i at position p >= carry (a target) looks at the entries before it.
// BLOCKS (csrc/lz4.hip, carry 0): the stream is cut into blocks of CFLZ_COSTBLK bytes that are matched as streams of
// their own -- a candidate in front of p's block ends the walk, as one outside the window does.
template <bool BLOCKS>
__device__ __forceinline__ void lz_match(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ keys,
	const uint32_t* __restrict__ pos, uint32_t pairs, uint32_t carry, uint32_t n, uint32_t* __restrict__ ld)
{
	const uint32_t i = blockIdx.x*256u + threadIdx.x;
	if (i >= pairs)
		return;
	const uint32_t p = pos[i];
	if (p < carry)
		return;
	const uint32_t key = keys[i];
	const uint32_t t = p - carry;
	uint32_t end = (t/CFLZ_CHUNK + 1u)*CFLZ_CHUNK;
	end = end < n ? end : n;
	uint32_t cap = end - t;                              // >= 1; p + cap <= carry + n
	cap = cap < (uint32_t)CFLZ_MAX ? cap : (uint32_t)CFLZ_MAX;
	uint32_t best = 0u, dist = 1u;
	for (uint32_t j = 1u; j <= (uint32_t)CFLZ_CANDS && j <= i; ++j) {
		if (keys[i - j] != key)
			break;
		const uint32_t q = pos[i - j];                   // q < p: the sort is stable
		if (p - q > CFLZ_WINDOW)
			break;
		if (BLOCKS && q < (p & ~(CFLZ_COSTBLK - 1u)))
			break;
		const uint8_t* a = bytes + p;
		const uint8_t* b = bytes + q;
		uint32_t len = 0u;
		bool open = true;
		while (len + 4u <= cap) {                        // reads a[len .. len + 3], all below p + cap
			const uint32_t x = lz_load32(a + len) ^ lz_load32(b + len);
			if (x) {
				len += (uint32_t)__builtin_ctz(x) >> 3;
				open = false;
				break;
			}
			len += 4u;
		}
		while (open && len < cap && a[len] == b[len])
			++len;
		if (len > best) {
			best = len;
			dist = p - q;
		}
		if (best == cap)
			break;
	}
	ld[t] = best ? (best | ((dist - 1u) << 16)) : 0u;
}

__global__ __launch_bounds__(256) void cfhip_lz_match_kernel(const uint8_t* __restrict__ bytes,
	const uint32_t* __restrict__ keys, const uint32_t* __restrict__ pos, uint32_t pairs, uint32_t carry, uint32_t n,
	uint32_t* __restrict__ ld)
{
	lz_match<false>(bytes, keys, pos, pairs, carry, n, ld);
}

// The match stage of the LZ4 encoder: every candidate inside the position's own block.
__global__ __launch_bounds__(256) void cfhip_lz4_match_kernel(const uint8_t* __restrict__ bytes,
	const uint32_t* __restrict__ keys, const uint32_t* __restrict__ pos, uint32_t pairs, uint32_t carry, uint32_t n,
	uint32_t* __restrict__ ld)
{
	lz_match<true>(bytes, keys, pos, pairs, carry, n, ld);
}

#define LZ_TAKEN CFLZ_TAKEN
#define LZ_SEEN CFLZ_SEEN

// One wavefront per chunk.  bytes: the slice's first TARGET byte.  LDS: 16 KiB of L / D and 1280 bytes of counters.
__global__ __launch_bounds__(64) void cfhip_lz_parse_kernel(const uint8_t* __restrict__ bytes,
	const uint32_t* __restrict__ ld, uint32_t n, uint32_t* __restrict__ hist)
{
	__shared__ uint32_t s_ld[CFLZ_CHUNK];
	__shared__ uint32_t s_h[CFLZ_HIST];
	const uint32_t lane = threadIdx.x;
	const uint32_t base = blockIdx.x*CFLZ_CHUNK;
	const uint32_t clen = n - base < CFLZ_CHUNK ? n - base : CFLZ_CHUNK;
	for (uint32_t i = lane*4u; i < CFLZ_CHUNK; i += 256u) {
		uint4 v = make_uint4(0u, 0u, 0u, 0u);
		if (i + 4u <= clen)
			v = *reinterpret_cast<const uint4*>(ld + base + i);      // base is a multiple of 4096 words
		else {
			if (i < clen) v.x = ld[base + i];
			if (i + 1u < clen) v.y = ld[base + i + 1u];
			if (i + 2u < clen) v.z = ld[base + i + 2u];
		}
		*reinterpret_cast<uint4*>(s_ld + i) = v;
	}
	for (uint32_t i = lane; i < (uint32_t)CFLZ_HIST; i += 64u)
		s_h[i] = 0u;
	__syncthreads();
	// one-step lazy: a match stands unless the next position's is longer.  A lane owns the 64 positions
	// lane + 64 t: it decides all of them from the staged words into one 64-bit mask, and writes the flags only after
	// the barrier, when no lane reads a neighbour's word any more.
	unsigned long long taken = 0ull;
	for (uint32_t t = 0u; t < CFLZ_CHUNK/64u; ++t) {
		const uint32_t i = lane + 64u*t;
		if (i >= clen)
			break;
		const uint32_t l = s_ld[i] & 0x1FFu;
		if (l >= (uint32_t)CFLZ_MIN) {
			const uint32_t next = i + 1u < clen ? s_ld[i + 1u] & 0x1FFu : 0u;
			if (next <= l)
				taken |= 1ull << t;
		}
	}
	__syncthreads();
	for (uint32_t t = 0u; t < CFLZ_CHUNK/64u && (taken >> t); ++t)
		if ((taken >> t) & 1ull)
			s_ld[lane + 64u*t] |= LZ_TAKEN;
	__syncthreads();
	if (lane == 0u) {
		uint32_t p = 0u;
		while (p < clen) {
			const uint32_t v = s_ld[p];
			s_ld[p] = v | LZ_SEEN;
			p += (v & LZ_TAKEN) ? (v & 0x1FFu) : 1u;
		}
	}
	__syncthreads();
	uint32_t extra = 0u, literals = 0u, matches = 0u, matched = 0u;
	for (uint32_t i = lane; i < clen; i += 64u) {
		const uint32_t v = s_ld[i];
		if (!(v & LZ_SEEN))
			continue;
		if (v & LZ_TAKEN) {
			uint32_t el, ed;
			const uint32_t len = v & 0x1FFu;
			const uint32_t lc = lz_length_code(len, &el);
			const uint32_t dc = lz_dist_code(v >> 16, &ed);
			atomicAdd(&s_h[257u + lc], 1u);
			atomicAdd(&s_h[(uint32_t)CFLZ_LL + dc], 1u);
			extra += el + ed;
			++matches;
			matched += len;
		} else {
			atomicAdd(&s_h[bytes[base + i]], 1u);
			++literals;
		}
	}
	if (extra) atomicAdd(&s_h[CFLZ_EXTRA], extra);
	if (literals) atomicAdd(&s_h[CFLZ_LITERALS], literals);
	if (matches) atomicAdd(&s_h[CFLZ_MATCHES], matches);
	if (matched) atomicAdd(&s_h[CFLZ_MATCHED], matched);
	__syncthreads();
	uint32_t* out = hist + (size_t)(base/CFLZ_COSTBLK)*CFLZ_HIST;
	for (uint32_t i = lane; i < (uint32_t)CFLZ_HIST; i += 64u) {
		const uint32_t v = s_h[i];
		if (v)
			atomicAdd(out + i, v);
	}
}

// log2(x) in 16.16 fixed point, x >= 1: lzsize_ref.lg16
__device__ __forceinline__ uint32_t lz_lg16(uint32_t x)
{
	const uint32_t e = 31u - (uint32_t)__builtin_clz(x);
	unsigned long long m = (unsigned long long)x << (31u - e);
	uint32_t f = 0u;
	for (int k = 0; k < 16; ++k) {
		m = (m*m) >> 31;
		f <<= 1;
		if (m >> 32) {
			f |= 1u;
			m >>= 1;
		}
	}
	return (e << 16) | f;
}

__device__ __forceinline__ unsigned long long lz_wave_sum(unsigned long long v)
{
	for (int s = 32; s; s >>= 1)
		v += __shfl_xor(v, s, 64);
	return v;
}

// sum of n (lg16(T) - lg16(n)) over one alphabet of `count` counters; eob: the symbol that occurs once more
__device__ __forceinline__ unsigned long long lz_entropy(const uint32_t* __restrict__ h, uint32_t count, uint32_t eob,
	uint32_t lane)
{
	unsigned long long total = 0ull;
	for (uint32_t i = lane; i < count; i += 64u)
		total += h[i] + (i == eob ? 1u : 0u);
	total = lz_wave_sum(total);
	if (!total)
		return 0ull;
	const uint32_t lt = lz_lg16((uint32_t)total);
	unsigned long long bits = 0ull;
	for (uint32_t i = lane; i < count; i += 64u) {
		const uint32_t v = h[i] + (i == eob ? 1u : 0u);
		if (v)
			bits += (unsigned long long)v*(lt - lz_lg16(v));
	}
	return lz_wave_sum(bits);
}

// One wavefront per cost block.
__global__ __launch_bounds__(64) void cfhip_lz_cost_kernel(const uint32_t* __restrict__ hist, unsigned long long* __restrict__ acc)
{
	const uint32_t lane = threadIdx.x;
	const uint32_t* h = hist + (size_t)blockIdx.x*CFLZ_HIST;
	unsigned long long bits = lz_entropy(h, CFLZ_LL, 256u, lane);
	bits += lz_entropy(h + CFLZ_LL, CFLZ_DD, 0xFFFFFFFFu, lane);
	if (lane == 0u) {
		atomicAdd(acc + 0, bits + ((unsigned long long)h[CFLZ_EXTRA] << 16));
		atomicAdd(acc + 1, (unsigned long long)h[CFLZ_LITERALS]);
		atomicAdd(acc + 2, (unsigned long long)h[CFLZ_MATCHES]);
		atomicAdd(acc + 3, (unsigned long long)h[CFLZ_MATCHED]);
	}
}

__global__ void cfhip_lz_final_kernel(const unsigned long long* __restrict__ acc, unsigned long long bytes_in,
	unsigned long long* __restrict__ out)
{
	if (threadIdx.x || blockIdx.x)
		return;
	const unsigned long long bits = acc[0];
	out[0] = bytes_in;
	out[1] = bits;
	out[2] = (bits + (8ull << 16) - 1ull)/(8ull << 16);
	out[3] = acc[1];
	out[4] = acc[2];
	out[5] = acc[3];
}

} // namespace

extern "C" hipError_t cfhip_lz_sort_bytes(size_t m, size_t* bytes)
{
	*bytes = 0;
	if (!m)
		return hipSuccess;
	uint32_t* none = nullptr;
	return rocprim::radix_sort_pairs(nullptr, *bytes, none, none, none, none, m, 0u, 32u, (hipStream_t)nullptr, false);
}

#define LZ_STAGE(k, body) do { \
		if (ev && (e = hipEventRecord(ev[2*(k)], stream)) != hipSuccess) return e; \
		body; \
		if ((e = hipGetLastError()) != hipSuccess) return e; \
		if (ev && (e = hipEventRecord(ev[2*(k) + 1], stream)) != hipSuccess) return e; \
	} while (0)

static hipError_t lz_launch_matches(uint8_t* base, const cflz_layout* lay, size_t sort_bytes, uint32_t carry,
	uint32_t n, bool blocks, hipEvent_t* ev, hipStream_t stream)
{
	const uint32_t m = carry + n;
	const uint32_t pairs = m >= 4u ? m - 3u : 0u;
	uint8_t* bytes = base + lay->bytes;
	uint32_t* keys_in = reinterpret_cast<uint32_t*>(base + lay->keys_in);
	uint32_t* keys_out = reinterpret_cast<uint32_t*>(base + lay->keys_out);
	uint32_t* pos_in = reinterpret_cast<uint32_t*>(base + lay->pos_in);
	uint32_t* pos_out = reinterpret_cast<uint32_t*>(base + lay->pos_out);
	uint32_t* ld = reinterpret_cast<uint32_t*>(base + lay->ld);
	hipError_t e = hipSuccess;
	LZ_STAGE(0, hipLaunchKernelGGL(cfhip_lz_keys_kernel, dim3((m + 255u)/256u), dim3(256), 0, stream, bytes, m, carry,
		keys_in, pos_in, ld));
	LZ_STAGE(1, {
		if (pairs) {
			size_t need = 0;
			e = rocprim::radix_sort_pairs(nullptr, need, keys_in, keys_out, pos_in, pos_out, pairs, 0u, 32u, stream, false);
			if (e == hipSuccess && need > sort_bytes)
				e = hipErrorOutOfMemory;
			if (e == hipSuccess) {
				need = sort_bytes;
				e = rocprim::radix_sort_pairs(base + lay->sort, need, keys_in, keys_out, pos_in, pos_out, pairs, 0u, 32u,
					stream, false);
			}
			if (e != hipSuccess)
				return e;
		}
	});
	LZ_STAGE(2, {
		if (pairs && blocks)
			hipLaunchKernelGGL(cfhip_lz4_match_kernel, dim3((pairs + 255u)/256u), dim3(256), 0, stream, bytes, keys_out,
				pos_out, pairs, carry, n, ld);
		else if (pairs)
			hipLaunchKernelGGL(cfhip_lz_match_kernel, dim3((pairs + 255u)/256u), dim3(256), 0, stream, bytes, keys_out,
				pos_out, pairs, carry, n, ld);
	});
	return hipSuccess;
}

extern "C" hipError_t cfhip_launch_lz_matches(uint8_t* base, const cflz_layout* lay, size_t sort_bytes, uint32_t carry,
	uint32_t n, hipEvent_t* ev, hipStream_t stream)
{
	return lz_launch_matches(base, lay, sort_bytes, carry, n, false, ev, stream);
}

extern "C" hipError_t cfhip_launch_lz_block_matches(uint8_t* base, const cflz_layout* lay, size_t sort_bytes, uint32_t n,
	hipEvent_t* ev, hipStream_t stream)
{
	return lz_launch_matches(base, lay, sort_bytes, 0u, n, true, ev, stream);
}

extern "C" hipError_t cfhip_launch_lz_slice(uint8_t* base, const cflz_layout* lay, size_t sort_bytes, uint32_t carry,
	uint32_t n, hipEvent_t* ev, hipStream_t stream)
{
	const uint32_t blocks = (n + CFLZ_COSTBLK - 1u)/CFLZ_COSTBLK, chunks = (n + CFLZ_CHUNK - 1u)/CFLZ_CHUNK;
	uint8_t* bytes = base + lay->bytes;
	uint32_t* ld = reinterpret_cast<uint32_t*>(base + lay->ld);
	uint32_t* hist = reinterpret_cast<uint32_t*>(base + lay->hist);
	unsigned long long* acc = reinterpret_cast<unsigned long long*>(base + lay->acc);
	hipError_t e = hipSuccess;
	if ((e = hipMemsetAsync(hist, 0, (size_t)blocks*CFLZ_HIST*4u, stream)) != hipSuccess)
		return e;
	if ((e = cfhip_launch_lz_matches(base, lay, sort_bytes, carry, n, ev, stream)) != hipSuccess)
		return e;
	LZ_STAGE(3, hipLaunchKernelGGL(cfhip_lz_parse_kernel, dim3(chunks), dim3(64), 0, stream, bytes + carry, ld, n, hist));
	LZ_STAGE(4, hipLaunchKernelGGL(cfhip_lz_cost_kernel, dim3(blocks), dim3(64), 0, stream, hist, acc));
	return hipSuccess;
}
#undef LZ_STAGE

extern "C" hipError_t cfhip_launch_lz_final(const unsigned long long* acc, unsigned long long bytes_in,
	unsigned long long* out, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_lz_final_kernel, dim3(1), dim3(64), 0, stream, acc, bytes_in, out);
	return hipGetLastError();
}
