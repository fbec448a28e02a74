// lz4.hip -- LZ4 frames of a byte stream on gfx950, both ways.  THE DEFINITION of every byte
// written and of every verdict given is tests/lz4_ref.py; these kernels return both exactly.
//
// ENCODE.  One slice (lz4.h) of whole 64 KiB blocks runs eight stages; `final` follows the last slice:
//   keys, sort, match   lzsize.hip's, the match stage with the block floor (cfhip_launch_lz_block_matches)
//   parse    one wavefront per chunk of 4096 bytes: lzsize.hip's lazy rule, then ONE LANE WALKS the chunk and lists its
//            matches, a match that follows one of the same distance without a literal between them added to it
//   plan     one workgroup per block: one thread joins the lists across the 15 chunk ends; all apply the rules of the
//            block's end, scan the matches' ends (where each sequence's literals start), the sequences' encoded sizes
//            and their number, write one record per sequence, and decide stored or compressed
//   offsets  one wavefront: scan of the blocks' bytes behind the running offset, the counters
//   emit     one workgroup per block: the size word; a thread writes a sequence's token, length bytes, short literal
//            run, offset; a wavefront copies a long literal run together.  A stored block is a copy
//   hash     one wavefront per block: XXH32 of the bytes as stored -- four lanes hold the four accumulators and read
//            the stripes the others staged in LDS -- behind the block
//   final    the header with its HC, the end mark, the result
// DECODE.  Three stages:
//   chain    one lane checks the header and walks the size words (a dependent chain of 4-byte loads), leaving per block
//            where its bytes lie
//   blocks   one wavefront per block: the stored bytes staged in LDS, XXH32 taken from there, then batches of 64
//            sequences: ONE LANE parses and range-checks them (lz4.h's cflz4_sequence, the host program's) into LDS
//            records; every lane copies one record's literals (a wavefront a long run); then the matches in sequence
//            order, byte i from start - offset + i mod offset.  The output is assembled in LDS and written out once
//            the block has passed: 128 KiB of the CU's 160, one workgroup per CU
//   final    the result from the lowest failing block
// A copy that reads what another copy wrote is separated from it by a barrier: literals before matches, each match
// before the next.  Nothing is read outside the frame or written outside [out, out + out_bytes): every length from
// the stream is checked by the one lane before any lane uses it.
#include "lz4.h"

namespace {

__device__ __forceinline__ uint32_t l4_load32(const uint8_t* p)
{
	uint32_t v;
	__builtin_memcpy(&v, p, 4);
	return v;
}

__device__ __forceinline__ uint32_t l4_wave_scan(uint32_t v, uint32_t lane)
{
	for (uint32_t s = 1u; s < 64u; s <<= 1) {
		const uint32_t o = __shfl_up(v, s, 64);
		if (lane >= s)
			v += o;
	}
	return v;
}

// bytes behind a length nibble: none below 15, then one per started 255
__device__ __forceinline__ uint32_t l4_ext(uint32_t v)
{
	return v >= 15u ? 1u + (v - 15u)/255u : 0u;
}

__device__ __forceinline__ uint8_t* l4_put_runs(uint8_t* p, uint32_t v)
{
	for (v -= 15u; v >= 255u; v -= 255u)
		*p++ = 255u;
	*p++ = (uint8_t)v;
	return p;
}

// ---- encode ----------------------------------------------------------------------------------------------------------
// One wavefront per chunk.  LDS: 16 KiB of L / D and 8 KiB of match records.
__global__ __launch_bounds__(64) void cfhip_lz4_parse_kernel(const uint32_t* __restrict__ ld, uint32_t n,
	uint32_t* __restrict__ mrec, uint32_t* __restrict__ mcount)
{
	__shared__ uint32_t s_ld[CFLZ_CHUNK];
	__shared__ uint32_t s_rec[2u*CFLZ4_CHUNK_MATCHES];
	__shared__ uint32_t s_cnt;
	const uint32_t lane = threadIdx.x;
	const uint32_t base = blockIdx.x*CFLZ_CHUNK;
	const uint32_t clen = n - base < CFLZ_CHUNK ? n - base : CFLZ_CHUNK;
	for (uint32_t i = lane*4u; i < CFLZ_CHUNK; i += 256u) {
		uint4 v = make_uint4(0u, 0u, 0u, 0u);
		if (i + 4u <= clen)
			v = *reinterpret_cast<const uint4*>(ld + base + i);
		else {
			if (i < clen) v.x = ld[base + i];
			if (i + 1u < clen) v.y = ld[base + i + 1u];
			if (i + 2u < clen) v.z = ld[base + i + 2u];
		}
		*reinterpret_cast<uint4*>(s_ld + i) = v;
	}
	__syncthreads();
	// one-step lazy, as cfhip_lz_parse_kernel has it: decided from the staged words, flagged after the barrier
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
			s_ld[lane + 64u*t] |= CFLZ_TAKEN;
	__syncthreads();
	if (lane == 0u) {
		const uint32_t in_block = (blockIdx.x % CFLZ4_CHUNKS)*CFLZ_CHUNK;
		uint32_t p = 0u, cnt = 0u, start = 0u, len = 0u, d1 = 0u;
		while (p < clen) {
			const uint32_t v = s_ld[p];
			if (v & CFLZ_TAKEN) {
				const uint32_t l = v & 0x1FFu;
				if (len && start + len == p && d1 == (v >> 16))
					len += l;
				else {
					if (len) {
						s_rec[2u*cnt] = (in_block + start) | ((d1 + 1u) << 16);
						s_rec[2u*cnt + 1u] = len;
						++cnt;
					}
					start = p;
					len = l;
					d1 = v >> 16;
				}
				p += l;
			} else
				++p;
		}
		if (len) {
			s_rec[2u*cnt] = (in_block + start) | ((d1 + 1u) << 16);
			s_rec[2u*cnt + 1u] = len;
			++cnt;
		}
		s_cnt = cnt;
	}
	__syncthreads();
	const uint32_t words = 2u*s_cnt;
	uint32_t* out = mrec + (size_t)blockIdx.x*2u*CFLZ4_CHUNK_MATCHES;
	for (uint32_t i = lane; i < words; i += 64u)
		out[i] = s_rec[i];
	if (lane == 0u)
		mcount[blockIdx.x] = s_cnt;
}

// exclusive scan over the 256 threads of a workgroup (sum, or max); *total: over all of them
template <bool MAX>
__device__ __forceinline__ uint32_t l4_block_scan(uint32_t v, uint32_t* s, uint32_t tid, uint32_t* total)
{
	s[tid] = v;
	__syncthreads();
	for (uint32_t o = 1u; o < 256u; o <<= 1) {
		const uint32_t x = tid >= o ? s[tid - o] : 0u;
		__syncthreads();
		if (tid >= o)
			s[tid] = MAX ? (s[tid] > x ? s[tid] : x) : s[tid] + x;
		__syncthreads();
	}
	const uint32_t excl = tid ? s[tid - 1u] : 0u;
	*total = s[255];
	__syncthreads();
	return excl;
}

// The rules of a block's end (lz4_ref.block_matches) on a match of `len` bytes at `start`: false: it becomes literals.
__device__ __forceinline__ bool l4_end_rules(uint32_t nb, uint32_t start, uint32_t* len)
{
	if (!*len || nb <= CFLZ4_MATCH_MARGIN || start > nb - CFLZ4_MATCH_MARGIN)
		return false;
	if (start + *len > nb - CFLZ4_LAST_LITERALS) {
		*len = nb - CFLZ4_LAST_LITERALS - start;
		if (*len < (uint32_t)CFLZ_MIN)
			return false;
	}
	return true;
}

// One workgroup of 256 threads per block.  A thread owns 64 consecutive slots of the block's 16 x 1024 match records.
__global__ __launch_bounds__(256) void cfhip_lz4_plan_kernel(uint32_t* mrec, const uint32_t* __restrict__ mcount,
	uint32_t n, uint4* __restrict__ seq, uint32_t* __restrict__ blk)
{
	__shared__ uint32_t s_cnt[CFLZ4_CHUNKS];
	__shared__ uint32_t s_scan[256];
	__shared__ uint32_t s_matched;
	const uint32_t tid = threadIdx.x, b = blockIdx.x;
	const uint32_t nb = n - b*CFLZ4_BLOCK < CFLZ4_BLOCK ? n - b*CFLZ4_BLOCK : CFLZ4_BLOCK;
	const uint32_t nch = (nb + CFLZ_CHUNK - 1u)/CFLZ_CHUNK;
	uint32_t* rec = mrec + (size_t)b*2u*CFLZ4_BLOCK_MATCHES;
	if (tid < CFLZ4_CHUNKS)
		s_cnt[tid] = tid < nch ? mcount[b*CFLZ4_CHUNKS + tid] : 0u;
	if (tid == 0u)
		s_matched = 0u;
	__syncthreads();
	// across the chunk ends: a chunk's first match, where it starts the chunk behind a match of the same distance that
	// ends the chunk before, is added to that one (a chunk that is one such match passes the chain on)
	if (tid == 0u) {
		uint32_t tail = 0xFFFFFFFFu;                            // slot of the last match so far
		for (uint32_t k = 0u; k < nch; ++k) {
			const uint32_t c = s_cnt[k];
			if (!c)
				continue;
			const uint32_t first = k*CFLZ4_CHUNK_MATCHES;
			uint32_t last = first + c - 1u;
			if (k && tail != 0xFFFFFFFFu) {
				const uint32_t t0 = rec[2u*tail], t1 = rec[2u*tail + 1u], f0 = rec[2u*first];
				if ((f0 & 0xFFFFu) == k*CFLZ_CHUNK && (t0 & 0xFFFFu) + t1 == k*CFLZ_CHUNK && (t0 >> 16) == (f0 >> 16)) {
					rec[2u*tail + 1u] = t1 + rec[2u*first + 1u];
					rec[2u*first + 1u] = 0u;
					if (c == 1u)
						last = tail;
				}
			}
			tail = last;
		}
	}
	__threadfence_block();
	__syncthreads();
	const uint32_t chunk = tid >> 4, idx0 = (tid & 15u)*64u, slot0 = tid*64u;
	const uint32_t have = s_cnt[chunk] > idx0 ? (s_cnt[chunk] - idx0 < 64u ? s_cnt[chunk] - idx0 : 64u) : 0u;
	// the end of the last match in front of each thread's slots
	uint32_t end = 0u;
	for (uint32_t j = 0u; j < have; ++j) {
		const uint32_t w0 = rec[2u*(slot0 + j)];
		uint32_t len = rec[2u*(slot0 + j) + 1u];
		if (l4_end_rules(nb, w0 & 0xFFFFu, &len))
			end = (w0 & 0xFFFFu) + len;
	}
	uint32_t last_end;
	const uint32_t prev_end = l4_block_scan<true>(end, s_scan, tid, &last_end);
	// the sequences' bytes and their number
	uint32_t bytes = 0u, count = 0u, matched = 0u, at = prev_end;
	for (uint32_t j = 0u; j < have; ++j) {
		const uint32_t w0 = rec[2u*(slot0 + j)], start = w0 & 0xFFFFu;
		uint32_t len = rec[2u*(slot0 + j) + 1u];
		if (!l4_end_rules(nb, start, &len))
			continue;
		const uint32_t lit = start - at;
		bytes += 1u + l4_ext(lit) + lit + 2u + l4_ext(len - 4u);
		++count;
		matched += len;
		at = start + len;
	}
	uint32_t total_bytes, total_count;
	uint32_t where = l4_block_scan<false>(bytes, s_scan, tid, &total_bytes);
	uint32_t index = l4_block_scan<false>(count, s_scan, tid, &total_count);
	if (matched)
		atomicAdd(&s_matched, matched);
	uint4* out = seq + (size_t)b*CFLZ4_BLOCK_MATCHES;
	at = prev_end;
	for (uint32_t j = 0u; j < have; ++j) {
		const uint32_t w0 = rec[2u*(slot0 + j)], start = w0 & 0xFFFFu;
		uint32_t len = rec[2u*(slot0 + j) + 1u];
		if (!l4_end_rules(nb, start, &len))
			continue;
		const uint32_t lit = start - at;
		out[index++] = make_uint4(where, at, start, len | (w0 & 0xFFFF0000u));    // len <= 65530, distance <= 32768
		where += 1u + l4_ext(lit) + lit + 2u + l4_ext(len - 4u);
		at = start + len;
	}
	__syncthreads();
	if (tid == 0u) {
		const uint32_t lit = nb - last_end;
		const uint32_t enc = total_bytes + 1u + l4_ext(lit) + lit;
		const uint32_t raw = enc >= nb ? 1u : 0u;
		uint32_t* r = blk + (size_t)b*CFLZ4_B_WORDS;
		r[CFLZ4_B_SIZE] = raw ? nb : enc;
		r[CFLZ4_B_RAW] = raw;
		r[CFLZ4_B_SEQS] = total_count;
		r[CFLZ4_B_TAIL] = last_end;
		r[CFLZ4_B_TAIL_OFF] = total_bytes;
		r[CFLZ4_B_MATCHED] = s_matched;
	}
}

// One wavefront: the blocks' offsets behind the running one, and the state.
__global__ __launch_bounds__(64) void cfhip_lz4_offsets_kernel(uint32_t* __restrict__ blk, uint32_t blocks, uint32_t n, int first,
	unsigned long long* __restrict__ state)
{
	const uint32_t lane = threadIdx.x;
	unsigned long long off = first ? (unsigned long long)CFLZ4_HEADER : state[CFLZ4_S_OFF];
	unsigned long long comp = 0ull, stored = 0ull, seqs = 0ull, lits = 0ull, matched = 0ull;
	for (uint32_t b0 = 0u; b0 < blocks; b0 += 64u) {
		const uint32_t b = b0 + lane;
		uint32_t* rec = blk + (size_t)b*CFLZ4_B_WORDS;
		const uint32_t size = b < blocks ? rec[CFLZ4_B_SIZE] + 8u : 0u;          // the size word and the checksum
		const uint32_t incl = l4_wave_scan(size, lane);
		if (b < blocks) {
			rec[CFLZ4_B_OFF] = (uint32_t)(off + incl - size);
			if (rec[CFLZ4_B_RAW])
				++stored;
			else {
				const uint32_t nb = n - b*CFLZ4_BLOCK < CFLZ4_BLOCK ? n - b*CFLZ4_BLOCK : CFLZ4_BLOCK;
				++comp;
				seqs += rec[CFLZ4_B_SEQS] + 1u;
				matched += rec[CFLZ4_B_MATCHED];
				lits += nb - rec[CFLZ4_B_MATCHED];
			}
		}
		off += __shfl(incl, 63, 64);
	}
	for (int s = 32; s; s >>= 1) {
		comp += __shfl_xor(comp, s, 64);
		stored += __shfl_xor(stored, s, 64);
		seqs += __shfl_xor(seqs, s, 64);
		lits += __shfl_xor(lits, s, 64);
		matched += __shfl_xor(matched, s, 64);
	}
	if (lane == 0u) {
		state[CFLZ4_S_OFF] = off;
		state[CFLZ4_S_COMPRESSED] = (first ? 0ull : state[CFLZ4_S_COMPRESSED]) + comp;
		state[CFLZ4_S_STORED] = (first ? 0ull : state[CFLZ4_S_STORED]) + stored;
		state[CFLZ4_S_SEQS] = (first ? 0ull : state[CFLZ4_S_SEQS]) + seqs;
		state[CFLZ4_S_LITERALS] = (first ? 0ull : state[CFLZ4_S_LITERALS]) + lits;
		state[CFLZ4_S_MATCHED] = (first ? 0ull : state[CFLZ4_S_MATCHED]) + matched;
	}
}

#define L4_SHORT_RUN 32u   // literal runs up to here are copied by the sequence's own lane

// One workgroup of 256 threads per block.  bytes: the slice's first byte.
__global__ __launch_bounds__(256) void cfhip_lz4_emit_kernel(const uint8_t* __restrict__ bytes, uint32_t n,
	const uint4* __restrict__ seq, const uint32_t* __restrict__ blk, uint8_t* __restrict__ out)
{
	const uint32_t tid = threadIdx.x, lane = tid & 63u, b = blockIdx.x;
	const uint32_t nb = n - b*CFLZ4_BLOCK < CFLZ4_BLOCK ? n - b*CFLZ4_BLOCK : CFLZ4_BLOCK;
	const uint32_t* rec = blk + (size_t)b*CFLZ4_B_WORDS;
	const uint32_t size = rec[CFLZ4_B_SIZE], raw = rec[CFLZ4_B_RAW];
	const uint8_t* src = bytes + (size_t)b*CFLZ4_BLOCK;
	uint8_t* dst = out + rec[CFLZ4_B_OFF];
	if (tid < 4u)
		dst[tid] = (uint8_t)((size | (raw ? CFLZ4_RAW : 0u)) >> (8u*tid));
	dst += 4;
	if (raw) {
		for (uint32_t i = tid; i < nb; i += 256u)
			dst[i] = src[i];
		return;
	}
	const uint32_t nseq = rec[CFLZ4_B_SEQS];
	const uint4* list = seq + (size_t)b*CFLZ4_BLOCK_MATCHES;
	for (uint32_t j0 = 0u; j0 < nseq; j0 += 256u) {                // uniform over the workgroup
		const uint32_t j = j0 + tid;
		uint32_t run_src = 0u, run_dst = 0u, run_len = 0u;
		if (j < nseq) {
			const uint4 s = list[j];
			const uint32_t lit = s.z - s.y, len = s.w & 0xFFFFu, dist = s.w >> 16;
			uint8_t* p = dst + s.x;
			*p++ = (uint8_t)(((lit < 15u ? lit : 15u) << 4) | (len - 4u < 15u ? len - 4u : 15u));
			if (lit >= 15u)
				p = l4_put_runs(p, lit);
			if (lit <= L4_SHORT_RUN)
				for (uint32_t i = 0u; i < lit; ++i)
					p[i] = src[s.y + i];
			else {
				run_src = s.y;
				run_dst = (uint32_t)(p - dst);
				run_len = lit;
			}
			p += lit;
			p[0] = (uint8_t)dist;
			p[1] = (uint8_t)(dist >> 8);
			if (len - 4u >= 15u)
				l4_put_runs(p + 2, len - 4u);
		}
		for (unsigned long long m = __ballot(run_len != 0u); m; m &= m - 1ull) {
			const int from = __ffsll((long long)m) - 1;
			const uint32_t a = __shfl(run_src, from, 64), d = __shfl(run_dst, from, 64), l = __shfl(run_len, from, 64);
			for (uint32_t i = lane; i < l; i += 64u)
				dst[d + i] = src[a + i];
		}
	}
	// the last sequence: literals only
	const uint32_t tail = rec[CFLZ4_B_TAIL], lit = nb - tail;
	uint8_t* p = dst + rec[CFLZ4_B_TAIL_OFF];
	if (tid == 0u) {
		*p = (uint8_t)((lit < 15u ? lit : 15u) << 4);
		if (lit >= 15u)
			l4_put_runs(p + 1, lit);
	}
	p += 1u + l4_ext(lit);
	for (uint32_t i = tid; i < lit; i += 256u)
		p[i] = src[tail + i];
}

// XXH32 of p[0 .. size) by one wavefront: lanes 0..3 hold the accumulators, all lanes stage 64 stripes at a time in `tile`
// (256 words).  aligned: p is an LDS array itself (the decoder's staged block) and is read in place.  -> the hash in lane 0.
__device__ __forceinline__ uint32_t l4_wave_xxh32(const uint8_t* p, uint32_t size, uint32_t* tile, uint32_t lane)
{
	const uint32_t stripes = size >> 4;
	uint32_t acc = cflz4_xxh_init(lane & 3u);
	for (uint32_t s0 = 0u; s0 < stripes; s0 += 64u) {
		const uint32_t cnt = stripes - s0 < 64u ? stripes - s0 : 64u;
		if (lane < cnt)
			for (uint32_t k = 0u; k < 4u; ++k)
				tile[4u*lane + k] = l4_load32(p + 16u*(s0 + lane) + 4u*k);
		__syncthreads();
		if (lane < 4u)
			for (uint32_t s = 0u; s < cnt; ++s)
				acc = cflz4_xxh_round(acc, tile[4u*s + lane]);
		__syncthreads();
	}
	const uint32_t v1 = __shfl(acc, 1, 64), v2 = __shfl(acc, 2, 64), v3 = __shfl(acc, 3, 64);
	uint32_t h = 0u;
	if (lane == 0u)
		h = cflz4_xxh_finish(stripes ? cflz4_xxh_merge(acc, v1, v2, v3) : CFLZ4_P5, p + 16u*stripes, size);
	return h;
}

// One wavefront per block.
__global__ __launch_bounds__(64) void cfhip_lz4_hash_kernel(const uint32_t* __restrict__ blk, uint8_t* __restrict__ out)
{
	__shared__ uint32_t s_tile[256];
	const uint32_t lane = threadIdx.x;
	const uint32_t* rec = blk + (size_t)blockIdx.x*CFLZ4_B_WORDS;
	const uint32_t size = rec[CFLZ4_B_SIZE];
	uint8_t* p = out + rec[CFLZ4_B_OFF] + 4u;
	const uint32_t h = l4_wave_xxh32(p, size, s_tile, lane);
	if (lane == 0u)
		for (uint32_t i = 0u; i < 4u; ++i)
			p[size + i] = (uint8_t)(h >> (8u*i));
}

__global__ void cfhip_lz4_final_kernel(const unsigned long long* __restrict__ state, unsigned long long bytes_in,
	uint8_t* __restrict__ out, unsigned long long* __restrict__ result)
{
	if (threadIdx.x || blockIdx.x)
		return;
	const unsigned long long off = state[CFLZ4_S_OFF];
	cflz4_write_header(out, bytes_in);
	for (uint32_t i = 0u; i < 4u; ++i)
		out[off + i] = 0u;
	result[0] = bytes_in;
	result[1] = off + 4ull;
	result[2] = state[CFLZ4_S_COMPRESSED];
	result[3] = state[CFLZ4_S_STORED];
	result[4] = state[CFLZ4_S_SEQS];
	result[5] = state[CFLZ4_S_LITERALS];
	result[6] = state[CFLZ4_S_MATCHED];
}

// ---- decode ----------------------------------------------------------------------------------------------------------
// One wavefront; lane 0 walks.  rec: per block (where its bytes lie: low, high; the size word; 0).
__global__ __launch_bounds__(64) void cfhip_lz4_chain_kernel(const uint8_t* __restrict__ z, unsigned long long bytes,
	unsigned long long out_bytes, uint4* __restrict__ rec, unsigned long long* __restrict__ state)
{
	if (threadIdx.x || blockIdx.x)
		return;
	for (uint32_t i = 0u; i < (uint32_t)CFLZ4_D_WORDS; ++i)
		state[i] = 0ull;
	state[CFLZ4_D_STATUS] = ~0ull;
	cflz4_header h;
	uint32_t e = cflz4_parse_header(z, bytes, out_bytes, &h);
	if (e != CFLZ4_OK) {
		state[CFLZ4_D_STATUS] = e;
		return;
	}
	state[CFLZ4_D_CHECKSUMS] = h.block_checksums | (h.content_checksum << 1);
	const unsigned long long blocks = (out_bytes + CFLZ4_BLOCK - 1u)/CFLZ4_BLOCK;
	uint64_t pos = h.length;
	for (unsigned long long b = 0ull; b < blocks; ++b) {
		uint64_t at = 0u;
		uint32_t size = 0u, raw = 0u;
		e = cflz4_next_block(z, bytes, h.block_checksums, &pos, &at, &size, &raw);
		if (e != CFLZ4_OK) {
			state[CFLZ4_D_STATUS] = (b << 3) | e;
			state[CFLZ4_D_GOOD] = b;
			return;
		}
		rec[b] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), size | (raw ? CFLZ4_RAW : 0u), 0u);
	}
	state[CFLZ4_D_GOOD] = blocks;
	e = cflz4_frame_end(z, bytes, h.content_checksum, pos);
	if (e != CFLZ4_OK)
		state[CFLZ4_D_STATUS] = (blocks << 3) | e;
}

#define L4_BATCH 64u       // sequences parsed by the one lane before every lane copies

// One wavefront per block.  LDS: the stored bytes (64 KiB + 16), the output (64 KiB), 64 records, one tile.
__global__ __launch_bounds__(64) void cfhip_lz4_block_kernel(const uint8_t* __restrict__ z, const uint4* __restrict__ rec,
	unsigned long long* __restrict__ state, uint8_t* __restrict__ out, unsigned long long out_bytes)
{
	__shared__ uint32_t s_in_words[CFLZ4_BLOCK/4u + 4u];
	__shared__ uint32_t s_out_words[CFLZ4_BLOCK/4u];
	__shared__ uint32_t s_rec[5u*L4_BATCH];
	__shared__ uint32_t s_tile[256];
	__shared__ uint32_t s_ctl[3];                                  // records in the batch, class, last batch
	const uint32_t lane = threadIdx.x, b = blockIdx.x;
	if ((unsigned long long)b >= state[CFLZ4_D_GOOD])
		return;                                                    // the chain never reached this block
	uint8_t* s_in = reinterpret_cast<uint8_t*>(s_in_words);
	uint8_t* s_out = reinterpret_cast<uint8_t*>(s_out_words);
	const uint4 r = rec[b];
	const uint8_t* src = z + ((unsigned long long)r.x | ((unsigned long long)r.y << 32));
	const uint32_t size = r.z & ~CFLZ4_RAW, raw = r.z >> 31;       // 1 <= size <= 65536, inside the frame: the chain checked
	const unsigned long long base = (unsigned long long)b*CFLZ4_BLOCK;
	const uint32_t want = out_bytes - base < CFLZ4_BLOCK ? (uint32_t)(out_bytes - base) : CFLZ4_BLOCK;
	for (uint32_t i = 4u*lane; i + 4u <= size; i += 256u)
		s_in_words[i >> 2] = l4_load32(src + i);
	if ((size & ~3u) + lane < size)
		s_in[(size & ~3u) + lane] = src[(size & ~3u) + lane];
	__syncthreads();
	uint32_t status = CFLZ4_OK;
	if (state[CFLZ4_D_CHECKSUMS] & 1ull) {
		const uint32_t h = l4_wave_xxh32(s_in, size, s_tile, lane);
		if (lane == 0u)
			s_ctl[1] = h == cflz4_le32(src + size) ? CFLZ4_OK : CFLZ4_E_CHECKSUM;
		__syncthreads();
		status = s_ctl[1];
		__syncthreads();
	}
	uint32_t seqs = 0u, lits = 0u, matched = 0u;                    // lane 0's
	const uint8_t* from = s_in;
	if (status == CFLZ4_OK && raw) {
		if (size != want)
			status = CFLZ4_E_SIZE;
	} else if (status == CFLZ4_OK) {
		from = s_out;
		uint32_t ip = 0u, op = 0u;                                  // lane 0's
		for (;;) {
			if (lane == 0u) {
				uint32_t cnt = 0u, e = CFLZ4_OK, done = 0u;
				while (cnt < L4_BATCH) {
					cflz4_seq s;
					e = cflz4_sequence(s_in, size, want, &ip, op, &s);
					if (e != CFLZ4_OK)
						break;
					uint32_t* q = s_rec + 5u*cnt;
					q[0] = s.lit_at; q[1] = s.lit_len; q[2] = op; q[3] = s.offset; q[4] = s.match_len;
					op += s.lit_len + s.match_len;
					++cnt;
					++seqs;
					lits += s.lit_len;
					matched += s.match_len;
					if (!s.match_len) {
						done = 1u;
						if (op != want)
							e = CFLZ4_E_SIZE;
						break;
					}
				}
				s_ctl[0] = cnt; s_ctl[1] = e; s_ctl[2] = done;
			}
			__syncthreads();
			const uint32_t cnt = s_ctl[0], done = s_ctl[2];
			status = s_ctl[1];
			if (status != CFLZ4_OK)
				break;                                             // uniform: every lane read the same word
			// literals: every range lies inside s_in and inside s_out[0 .. want) (cflz4_sequence)
			uint32_t run_src = 0u, run_dst = 0u, run_len = 0u;
			if (lane < cnt) {
				const uint32_t* q = s_rec + 5u*lane;
				if (q[1] <= L4_SHORT_RUN)
					for (uint32_t i = 0u; i < q[1]; ++i)
						s_out[q[2] + i] = s_in[q[0] + i];
				else {
					run_src = q[0]; run_dst = q[2]; run_len = q[1];
				}
			}
			for (unsigned long long m = __ballot(run_len != 0u); m; m &= m - 1ull) {
				const int k = __ffsll((long long)m) - 1;
				const uint32_t a = __shfl(run_src, k, 64), d = __shfl(run_dst, k, 64), l = __shfl(run_len, k, 64);
				for (uint32_t i = lane; i < l; i += 64u)
					s_out[d + i] = s_in[a + i];
			}
			__syncthreads();                                       // the literals are in place before a match reads them
			for (uint32_t k = 0u; k < cnt; ++k) {
				const uint32_t* q = s_rec + 5u*k;
				const uint32_t off = q[3], ml = q[4], d = q[2] + q[1];
				if (!ml)
					break;
				if (off >= ml)
					for (uint32_t i = lane; i < ml; i += 64u)
						s_out[d + i] = s_out[d - off + i];
				else
					for (uint32_t i = lane; i < ml; i += 64u)
						s_out[d + i] = s_out[d - off + i % off];       // the source lies in front of d: complete
				__syncthreads();                                   // this match is in place before the next one reads it
			}
			if (done)
				break;
			__syncthreads();                                       // the records are read before lane 0 writes the next batch
		}
	}
	if (status != CFLZ4_OK) {
		if (lane == 0u)
			atomicMin(&state[CFLZ4_D_STATUS], ((unsigned long long)b << 3) | status);
		return;
	}
	__syncthreads();
	// the block has passed: want bytes to out + base (out is 4-byte aligned, base a multiple of 65536)
	uint32_t* dst = reinterpret_cast<uint32_t*>(out + base);
	const uint32_t* words = reinterpret_cast<const uint32_t*>(from);
	for (uint32_t i = lane; i < (want >> 2); i += 64u)
		dst[i] = words[i];
	if ((want & ~3u) + lane < want)
		out[base + (want & ~3u) + lane] = from[(want & ~3u) + lane];
	if (lane == 0u) {
		atomicAdd(&state[raw ? CFLZ4_D_STORED : CFLZ4_D_COMPRESSED], 1ull);
		if (!raw) {
			atomicAdd(&state[CFLZ4_D_SEQS], (unsigned long long)seqs);
			atomicAdd(&state[CFLZ4_D_LITERALS], (unsigned long long)lits);
			atomicAdd(&state[CFLZ4_D_MATCHED], (unsigned long long)matched);
		}
	}
}

__global__ void cfhip_lz4_dfinal_kernel(const unsigned long long* __restrict__ state, unsigned long long bytes,
	unsigned long long out_bytes, unsigned long long* __restrict__ result)
{
	if (threadIdx.x || blockIdx.x)
		return;
	const unsigned long long st = state[CFLZ4_D_STATUS];
	const bool ok = st == ~0ull;
	result[0] = bytes;
	result[1] = ok ? out_bytes : 0ull;
	result[2] = ok ? state[CFLZ4_D_COMPRESSED] : 0ull;
	result[3] = ok ? state[CFLZ4_D_STORED] : 0ull;
	result[4] = ok ? state[CFLZ4_D_SEQS] : 0ull;
	result[5] = ok ? state[CFLZ4_D_LITERALS] : 0ull;
	result[6] = ok ? state[CFLZ4_D_MATCHED] : 0ull;
	result[7] = ok ? 0ull : (st & 7ull) | ((st >> 3) << 32);       // status, bad_block
	result[8] = state[CFLZ4_D_CHECKSUMS] >> 1;                     // content_checksum, reserved
}

} // namespace

#define L4_STAGE(k, ...) do { \
		if (ev && (e = hipEventRecord(ev[2*(k)], stream)) != hipSuccess) return e; \
		hipLaunchKernelGGL(__VA_ARGS__); \
		if ((e = hipGetLastError()) != hipSuccess) return e; \
		if (ev && (e = hipEventRecord(ev[2*(k) + 1], stream)) != hipSuccess) return e; \
	} while (0)

extern "C" hipError_t cfhip_launch_lz4_slice(uint8_t* base, const cflz4_layout* lay, size_t sort_bytes, uint32_t n, int first,
	uint8_t* out, hipEvent_t* ev, hipStream_t stream)
{
	const uint32_t blocks = (n + CFLZ4_BLOCK - 1u)/CFLZ4_BLOCK, chunks = (n + CFLZ_CHUNK - 1u)/CFLZ_CHUNK;
	const uint8_t* bytes = base + lay->lz.bytes;
	uint32_t* ld = reinterpret_cast<uint32_t*>(base + lay->lz.ld);
	uint32_t* mrec = reinterpret_cast<uint32_t*>(base + lay->mrec);
	uint32_t* mcount = reinterpret_cast<uint32_t*>(base + lay->mcount);
	uint4* seq = reinterpret_cast<uint4*>(base + lay->seq);
	uint32_t* blk = reinterpret_cast<uint32_t*>(base + lay->blk);
	unsigned long long* state = reinterpret_cast<unsigned long long*>(base + lay->state);
	hipError_t e = cfhip_launch_lz_block_matches(base, &lay->lz, sort_bytes, n, ev, stream);
	if (e != hipSuccess)
		return e;
	L4_STAGE(3, cfhip_lz4_parse_kernel, dim3(chunks), dim3(64), 0, stream, ld, n, mrec, mcount);
	L4_STAGE(4, cfhip_lz4_plan_kernel, dim3(blocks), dim3(256), 0, stream, mrec, mcount, n, seq, blk);
	L4_STAGE(5, cfhip_lz4_offsets_kernel, dim3(1), dim3(64), 0, stream, blk, blocks, n, first, state);
	L4_STAGE(6, cfhip_lz4_emit_kernel, dim3(blocks), dim3(256), 0, stream, bytes, n, seq, blk, out);
	L4_STAGE(7, cfhip_lz4_hash_kernel, dim3(blocks), dim3(64), 0, stream, blk, out);
	return hipSuccess;
}

extern "C" hipError_t cfhip_launch_lz4_final(const unsigned long long* state, unsigned long long bytes_in, uint8_t* out,
	unsigned long long* result, hipEvent_t* ev, hipStream_t stream)
{
	hipError_t e = hipSuccess;
	L4_STAGE(0, cfhip_lz4_final_kernel, dim3(1), dim3(64), 0, stream, state, bytes_in, out, result);
	return hipSuccess;
}

extern "C" hipError_t cfhip_launch_lz4_decode(uint8_t* base, const cflz4_dlayout* lay, const uint8_t* z, unsigned long long bytes,
	uint8_t* out, unsigned long long out_bytes, unsigned long long* result, hipEvent_t* ev, hipStream_t stream)
{
	const uint32_t blocks = (uint32_t)((out_bytes + CFLZ4_BLOCK - 1u)/CFLZ4_BLOCK);
	uint4* rec = reinterpret_cast<uint4*>(base + lay->rec);
	unsigned long long* state = reinterpret_cast<unsigned long long*>(base + lay->state);
	hipError_t e = hipSuccess;
	L4_STAGE(0, cfhip_lz4_chain_kernel, dim3(1), dim3(64), 0, stream, z, bytes, out_bytes, rec, state);
	if (ev && (e = hipEventRecord(ev[2], stream)) != hipSuccess)
		return e;
	if (blocks) {
		hipLaunchKernelGGL(cfhip_lz4_block_kernel, dim3(blocks), dim3(64), 0, stream, z, rec, state, out, out_bytes);
		if ((e = hipGetLastError()) != hipSuccess)
			return e;
	}
	if (ev && (e = hipEventRecord(ev[3], stream)) != hipSuccess)
		return e;
	L4_STAGE(2, cfhip_lz4_dfinal_kernel, dim3(1), dim3(64), 0, stream, state, bytes, out_bytes, result);
	return hipSuccess;
}
#undef L4_STAGE
