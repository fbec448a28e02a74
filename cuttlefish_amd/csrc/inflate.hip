// inflate.hip -- indexed zlib streams back to their bytes on gfx950.  THE DEFINITION of the
// verdict and of the counters is tests/inflate_ref.py; the decode logic is inflate.h's, which tools/inflate_host.cpp
// runs on the CPU.
//
// One slice (inflate.h) runs four stages on one stream:
//   decode   one wavefront per chunk of 4096 output bytes, from the chunk's index entry: the lanes build the block's
//            decode tables in LDS, ONE LANE walks the bits and leaves a token word at each token's first position, then
//            every lane expands 64 positions into one word per output byte: the byte, or a pointer to the output
//            position whose byte it is, always below its own.  A failing chunk lowers the state's FAIL word
//   resolve  pointer jumping from one word array to the other, S'[i] = S[S[i]] while S[i] is a pointer: after round r
//            every position below 2^r is a byte, so ceil(log2 n) + 1 rounds are enqueued; each counts the pointers it
//            left, and a round returns at once when the one before left none.  A pointer into an earlier slice reads
//            the byte, final by then, from the output.  Runs only when no chunk failed
//   pack     one wavefront per chunk: the words of the array the last working round wrote, narrowed to bytes, and the
//            chunk's two Adler sums
//   fold     one wavefront: the chunks' sums behind the state's, the rounds that did work
// and after the last slice a final kernel compares the Adler-32 with the trailer's and fills cfhip_inflate_result.
// No wavefront waits for another: every dependency is a kernel boundary.  Every loop over bits or tokens consumes bits
// of the stream or produces bytes of the chunk; every read of the stream, the index and the words is range-checked;
// every store is an ordinary vector store or an atomic of the vector memory path.
#include "inflate.h"
#include "deflate.h"

namespace {

#define INF_NONE 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ uint32_t inf_wave_sum(uint32_t v)
{
	for (int s = 32; s; s >>= 1)
		v += __shfl_xor(v, s, 64);
	return v;
}

// One wavefront per chunk.  chunk0: the slice's first chunk; chunks: those of the whole output (0: the walk of an
// empty stream).  S: the slice's first word array.
__global__ __launch_bounds__(64) void cfhip_inflate_decode_kernel(const uint8_t* __restrict__ z, unsigned long long zbytes,
	const cfinf_entry* __restrict__ index, unsigned long long out_bytes, unsigned long long chunk0,
	unsigned long long chunks, uint32_t* __restrict__ S, unsigned long long* __restrict__ state)
{
	__shared__ CfinfWork w;
	const uint32_t lane = threadIdx.x;
	const unsigned long long c = chunk0 + blockIdx.x, base = c*CFINF_CHUNK;
	const uint32_t want = chunks ? (uint32_t)(out_bytes - base < CFINF_CHUNK ? out_bytes - base : CFINF_CHUNK) : 0u;
	const uint32_t err = cfinf_chunk(w, z, zbytes, index, chunks, c, want, lane, 64u);
	if (err != CFINF_OK) {
		if (lane == 0u)
			atomicMin(&state[CFINF_S_FAIL], (c << 3) | err);
		return;
	}
	// a lane owns the 64 positions from 64 lane on; the token that covers the first one may start before them
	const uint32_t first = 64u*lane;
	uint32_t p0 = 0u, t = 0u;
	if (first < want) {
		p0 = w.cover[lane];
		t = w.S[CFINF_PAD(p0)];
	}
	__syncthreads();
	uint32_t pointers = 0u;
	if (first < want) {
		uint32_t end = p0 + ((t & CFINF_MATCH) ? (t & 0xFFu) + 3u : 1u);
		const uint32_t stop = first + 64u < want ? first + 64u : want;
		for (uint32_t i = first; i < stop; ++i) {
			if (i == end) {
				p0 = i;
				t = w.S[CFINF_PAD(i)];
				end = p0 + ((t & CFINF_MATCH) ? (t & 0xFFu) + 3u : 1u);
			}
			const uint32_t v = cfinf_expand(t, p0, i, base);
			pointers += v >> 31;
			w.S[CFINF_PAD(i)] = v;
		}
	}
	__syncthreads();
	uint32_t* dst = S + (size_t)blockIdx.x*CFINF_CHUNK;
	for (uint32_t i = lane; i < want; i += 64u)
		dst[i] = w.S[CFINF_PAD(i)];
	pointers = inf_wave_sum(pointers);
	if (lane == 0u) {
		if (pointers) atomicAdd(&state[CFINF_S_LEFT], (unsigned long long)pointers);
		if (w.literals) atomicAdd(&state[CFINF_S_LITERALS], (unsigned long long)w.literals);
		if (w.matches) atomicAdd(&state[CFINF_S_MATCHES], (unsigned long long)w.matches);
		if (w.matched) atomicAdd(&state[CFINF_S_MATCHED], (unsigned long long)w.matched);
	}
}

// Round r >= 1 over the n words of a slice whose first output position is `at`: src -> dst, 16 words per thread (a
// workgroup adds once to the round's count: 4096 words per addition to one address).
#define INF_RESOLVE_PER 16u
__global__ __launch_bounds__(256) void cfhip_inflate_resolve_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
	uint32_t n, unsigned long long at, const uint8_t* __restrict__ out, unsigned long long* __restrict__ state, uint32_t r)
{
	__shared__ uint32_t s_left[4];
	if (state[CFINF_S_FAIL] != INF_NONE || state[CFINF_S_LEFT + r - 1u] == 0ull)
		return;
	uint32_t left = 0u;
	for (uint32_t k = 0u; k < INF_RESOLVE_PER; ++k) {
		const uint32_t i = (blockIdx.x*INF_RESOLVE_PER + k)*256u + threadIdx.x;
		if (i >= n)
			break;
		uint32_t v = src[i];
		if (v & CFINF_PTR) {
			const unsigned long long q = v & ~CFINF_PTR;
			if (q >= at + i)
				v = 0u;                                   // never written by the decode stage
			else if (q < at)
				v = out[q];                               // an earlier slice: final
			else
				v = src[q - at];
			left += v >> 31;
		}
		dst[i] = v;
	}
	left = inf_wave_sum(left);
	if ((threadIdx.x & 63u) == 0u)
		s_left[threadIdx.x >> 6] = left;
	__syncthreads();
	if (threadIdx.x == 0u) {
		const uint32_t still = s_left[0] + s_left[1] + s_left[2] + s_left[3];
		if (still)
			atomicAdd(&state[CFINF_S_LEFT + r], (unsigned long long)still);
	}
}

// the rounds that did work in the current slice: the first r whose count of pointers left is 0
__device__ __forceinline__ uint32_t inf_rounds(const unsigned long long* state, uint32_t bound)
{
	uint32_t r = 0u;
	while (r < bound && state[CFINF_S_LEFT + r] != 0ull)
		++r;
	return r;
}

// One wavefront per chunk of the slice: n words -> bytes at out (the slice's first byte, 4-byte aligned), the chunk's
// Adler sums as deflate.hip's adler stage leaves them.
__global__ __launch_bounds__(64) void cfhip_inflate_pack_kernel(const uint32_t* __restrict__ s0, const uint32_t* __restrict__ s1,
	uint32_t n, uint32_t bound, uint8_t* __restrict__ out, const unsigned long long* __restrict__ state,
	uint32_t* __restrict__ adler)
{
	if (state[CFINF_S_FAIL] != INF_NONE)
		return;
	const uint32_t* src = (inf_rounds(state, bound) & 1u) ? s1 : s0;
	const uint32_t lane = threadIdx.x;
	const uint32_t base = blockIdx.x*CFINF_CHUNK;
	const uint32_t clen = n - base < CFINF_CHUNK ? n - base : CFINF_CHUNK;
	uint32_t a = 0u, b = 0u;                                     // a lane sums 64 bytes: below 2^27
	for (uint32_t i = lane*4u; i < clen; i += 256u) {
		if (i + 4u <= clen) {
			const uint4 v = *reinterpret_cast<const uint4*>(src + base + i);
			const uint32_t b0 = v.x & 0xFFu, b1 = v.y & 0xFFu, b2 = v.z & 0xFFu, b3 = v.w & 0xFFu;
			*reinterpret_cast<uint32_t*>(out + base + i) = b0 | b1 << 8 | b2 << 16 | b3 << 24;
			a += b0 + b1 + b2 + b3;
			b += (clen - i)*b0 + (clen - i - 1u)*b1 + (clen - i - 2u)*b2 + (clen - i - 3u)*b3;
		} else
			for (uint32_t j = i; j < clen; ++j) {
				const uint32_t v = src[base + j] & 0xFFu;
				out[base + j] = (uint8_t)v;
				a += v;
				b += (clen - j)*v;
			}
	}
	unsigned long long ta = a, tb = b;
	for (int s = 32; s; s >>= 1) {
		ta += __shfl_xor(ta, s, 64);
		tb += __shfl_xor(tb, s, 64);
	}
	if (lane == 0u) {
		adler[2u*blockIdx.x] = (uint32_t)(ta % 65521ull);
		adler[2u*blockIdx.x + 1u] = (uint32_t)(tb % 65521ull);
	}
}

// One wavefront: the slice's chunk sums behind the state's (deflate.hip's combine rule), the slice's rounds.
__global__ __launch_bounds__(64) void cfhip_inflate_fold_kernel(const uint32_t* __restrict__ adler, uint32_t n, uint32_t bound,
	unsigned long long* __restrict__ state)
{
	__shared__ uint32_t s_a[64], s_b[64], s_l[64];
	if (state[CFINF_S_FAIL] != INF_NONE)
		return;
	const uint32_t lane = threadIdx.x;
	const uint32_t chunks = (n + CFINF_CHUNK - 1u)/CFINF_CHUNK, per = (chunks + 63u)/64u;
	const uint32_t c0 = lane*per < chunks ? lane*per : chunks, c1 = c0 + per < chunks ? c0 + per : chunks;
	unsigned long long A = 0ull, B = 0ull, L = 0ull;
	for (uint32_t c = c0; c < c1; ++c) {
		const uint32_t len = n - c*CFINF_CHUNK < CFINF_CHUNK ? n - c*CFINF_CHUNK : CFINF_CHUNK;
		B = (B + len*A + adler[2u*c + 1u]) % 65521ull;
		A = (A + adler[2u*c]) % 65521ull;
		L = (L + len) % 65521ull;
	}
	s_a[lane] = (uint32_t)A;
	s_b[lane] = (uint32_t)B;
	s_l[lane] = (uint32_t)L;
	__syncthreads();
	if (lane == 0u) {
		A = state[CFINF_S_A];
		B = state[CFINF_S_B];
		L = state[CFINF_S_LEN];
		for (uint32_t i = 0u; i < 64u; ++i) {
			B = (B + (unsigned long long)s_l[i]*A + s_b[i]) % 65521ull;
			A = (A + s_a[i]) % 65521ull;
			L = (L + s_l[i]) % 65521ull;
		}
		state[CFINF_S_A] = A;
		state[CFINF_S_B] = B;
		state[CFINF_S_LEN] = L;
		const unsigned long long r = inf_rounds(state, bound);
		if (r > state[CFINF_S_ROUNDS])
			state[CFINF_S_ROUNDS] = r;
	}
}

// The seven words of cfhip_inflate_result.
__global__ void cfhip_inflate_final_kernel(const unsigned long long* __restrict__ state, const uint8_t* __restrict__ z,
	unsigned long long zbytes, unsigned long long out_bytes, unsigned long long* __restrict__ result)
{
	if (threadIdx.x || blockIdx.x)
		return;
	const unsigned long long fail = state[CFINF_S_FAIL];
	const unsigned long long chunks = (out_bytes + CFINF_CHUNK - 1u)/CFINF_CHUNK;
	uint32_t status = 0u, bad = 0u, adler = 0u;
	if (fail != INF_NONE) {
		status = (uint32_t)(fail & 7u);
		bad = (uint32_t)(fail >> 3);
	} else {
		const uint32_t a = (uint32_t)((1ull + state[CFINF_S_A]) % 65521ull);
		const uint32_t b = (uint32_t)((state[CFINF_S_B] + state[CFINF_S_LEN]) % 65521ull);
		adler = (b << 16) | a;
		// (a stream that passed its wrapper checks holds six bytes or more)
		const uint32_t stored = zbytes < 4u ? ~adler : (uint32_t)z[zbytes - 4u] << 24 | (uint32_t)z[zbytes - 3u] << 16 |
			(uint32_t)z[zbytes - 2u] << 8 | (uint32_t)z[zbytes - 1u];
		if (stored != adler) {
			status = CFINF_E_CHECKSUM;
			bad = (uint32_t)(chunks ? chunks - 1u : 0u);
		}
	}
	const bool ok = status == 0u;
	result[0] = zbytes;
	result[1] = ok ? out_bytes : 0ull;
	result[2] = ok ? state[CFINF_S_LITERALS] : 0ull;
	result[3] = ok ? state[CFINF_S_MATCHES] : 0ull;
	result[4] = ok ? state[CFINF_S_MATCHED] : 0ull;
	result[5] = (unsigned long long)(ok ? adler : 0u) | (unsigned long long)status << 32;
	result[6] = (unsigned long long)bad | (ok ? state[CFINF_S_ROUNDS] : 0ull) << 32;
}

// One thread per chunk of a slice the encoder has just written: its entry from the group's record.
__global__ __launch_bounds__(256) void cfhip_zindex_kernel(const uint32_t* __restrict__ blk, uint32_t n,
	cfinf_entry* __restrict__ index)
{
	const uint32_t j = blockIdx.x*256u + threadIdx.x;
	if (j >= (n + CFLZ_CHUNK - 1u)/CFLZ_CHUNK)
		return;
	const uint32_t b = j/CFDF_CHUNKS, c = j % CFDF_CHUNKS;
	const uint32_t* rec = blk + (size_t)b*CFDF_B_WORDS;
	const unsigned long long off = rec[CFDF_B_OFF];
	cfinf_entry e;
	if (rec[CFDF_B_FORM] == 0u) {
		// stored: one block per 32768 bytes, five header bytes each
		const uint32_t sub = c >= CFDF_STORED_SPLIT/CFLZ_CHUNK ? 1u : 0u;
		e.header_bit = 8ull*(off + sub*(CFDF_STORED_SPLIT + 5u));
		e.token_bit = 8ull*(off + 5u*(1u + sub) + (unsigned long long)c*CFLZ_CHUNK);
	} else {
		e.header_bit = 8ull*off;
		e.token_bit = 8ull*off + rec[CFDF_B_CHUNK_BIT + c];
	}
	index[j] = e;
}

} // namespace

extern "C" hipError_t cfhip_launch_inflate_slice(uint8_t* base, const cfinf_layout* lay, const uint8_t* z, size_t zbytes,
	const cfinf_entry* index, size_t out_bytes, size_t at, uint32_t n, int first, uint8_t* out, hipEvent_t* ev,
	hipStream_t stream)
{
	static_assert(CFINF_CHUNK == CFLZ_CHUNK, "an index entry per chunk of the encoder");
	uint32_t* s0 = reinterpret_cast<uint32_t*>(base + lay->s0);
	uint32_t* s1 = reinterpret_cast<uint32_t*>(base + lay->s1);
	uint32_t* adler = reinterpret_cast<uint32_t*>(base + lay->adler);
	unsigned long long* state = reinterpret_cast<unsigned long long*>(base + lay->state);
	const unsigned long long chunks_all = (out_bytes + CFINF_CHUNK - 1u)/CFINF_CHUNK;
	const uint32_t chunks = n ? (n + CFINF_CHUNK - 1u)/CFINF_CHUNK : 1u;     // n == 0: the walk of an empty stream
	const uint32_t bound = n ? cfinf_rounds_bound(n) : 0u;
	hipError_t e;
	if (first) {
		if ((e = hipMemsetAsync(state, 0, CFINF_S_WORDS*8u, stream)) != hipSuccess) return e;
		if ((e = hipMemsetAsync(state + CFINF_S_FAIL, 0xFF, 8u, stream)) != hipSuccess) return e;
	} else if ((e = hipMemsetAsync(state + CFINF_S_LEFT, 0, (CFINF_MAX_ROUNDS + 1u)*8u, stream)) != hipSuccess)
		return e;
#define INF_EVENT(k) do { if (ev && (e = hipEventRecord(ev[k], stream)) != hipSuccess) return e; } while (0)
#define INF_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); if ((e = hipGetLastError()) != hipSuccess) return e; } while (0)
	INF_EVENT(0);
	INF_LAUNCH(cfhip_inflate_decode_kernel, dim3(chunks), dim3(64), 0, stream, z, (unsigned long long)zbytes, index,
		(unsigned long long)out_bytes, (unsigned long long)(at/CFINF_CHUNK), chunks_all, s0, state);
	INF_EVENT(1);
	INF_EVENT(2);
	for (uint32_t r = 1u; r <= bound; ++r)
		INF_LAUNCH(cfhip_inflate_resolve_kernel, dim3((n + 256u*INF_RESOLVE_PER - 1u)/(256u*INF_RESOLVE_PER)), dim3(256), 0, stream, (r & 1u) ? s0 : s1,
			(r & 1u) ? s1 : s0, n, (unsigned long long)at, out, state, r);
	INF_EVENT(3);
	INF_EVENT(4);
	if (n)
		INF_LAUNCH(cfhip_inflate_pack_kernel, dim3(chunks), dim3(64), 0, stream, s0, s1, n, bound, out + at, state, adler);
	INF_EVENT(5);
	INF_EVENT(6);
	if (n)
		INF_LAUNCH(cfhip_inflate_fold_kernel, dim3(1), dim3(64), 0, stream, adler, n, bound, state);
	INF_EVENT(7);
#undef INF_EVENT
#undef INF_LAUNCH
	return hipSuccess;
}

extern "C" hipError_t cfhip_launch_inflate_final(const unsigned long long* state, const uint8_t* z, size_t zbytes,
	size_t out_bytes, unsigned long long* result, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_inflate_final_kernel, dim3(1), dim3(64), 0, stream, state, z, (unsigned long long)zbytes,
		(unsigned long long)out_bytes, result);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_zindex(const uint32_t* blk, uint32_t n, size_t chunk0, cfinf_entry* index,
	hipStream_t stream)
{
	const uint32_t chunks = (n + CFLZ_CHUNK - 1u)/CFLZ_CHUNK;
	hipLaunchKernelGGL(cfhip_zindex_kernel, dim3((chunks + 255u)/256u), dim3(256), 0, stream, blk, n, index + chunk0);
	return hipGetLastError();
}
