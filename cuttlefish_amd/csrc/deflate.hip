// deflate.hip -- the zlib stream of a byte stream on gfx950.  THE DEFINITION of the bytes is
// tests/deflate_ref.py; these kernels write them exactly.  The tokens are the estimator's: the keys, sort and match
// stages are csrc/lzsize.hip's own (cfhip_launch_lz_matches), and the parse below is its parse with a record.
//
// One slice (deflate.h) runs eight stages on one stream:
//   keys, sort, match   lzsize.hip
//   parse    one wavefront per chunk of 4096 bytes: lzsize.hip's parse; it writes the flagged words back (a literal's
//            byte in bits 16..23), and the chunk's 320 counters to the chunk's own row (no atomics, nothing to clear)
//   adler    one wavefront per chunk: sum of the bytes and of (bytes to the chunk's end) x byte, mod 65521
//   codes    one wavefront per group of 65536 bytes: the group's counters, the length-limited code lengths of both
//            alphabets, the code-table header, the exact size of the three forms, the form, the bit at which every
//            chunk's tokens start.  The rank sort is parallel; ONE LANE merges, walks the tree and writes the header
//   offsets  one wavefront: scan of the groups' bytes behind the running offset, the Adler sums combined, the counters
//   emit     one wavefront per chunk: token bit lengths, an in-wave scan, the bits OR-ed into LDS, whole words copied
//            out; only the first and the last word of a chunk's bits, which a neighbour may share, go out as atomic ORs
//            (the buffer starts zeroed).  A stored group is a copy.
// Nothing is read back between the stages or the slices: the running offset, the Adler sums and the counters live in
// the scratch's state words.
#include "deflate.h"

namespace {

__constant__ unsigned char df_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t df_load32(const uint8_t* p)
{
	uint32_t v;
	__builtin_memcpy(&v, p, 4);
	return v;
}

__device__ __forceinline__ uint32_t df_wave_sum(uint32_t v)
{
	for (int s = 32; s; s >>= 1)
		v += __shfl_xor(v, s, 64);
	return v;
}

// inclusive prefix sum over the wavefront
__device__ __forceinline__ uint32_t df_wave_scan(uint32_t v, uint32_t lane)
{
	for (uint32_t s = 1u; s < 64u; s <<= 1) {
		const uint32_t o = __shfl_up(v, s, 64);
		if (lane >= s)
			v += o;
	}
	return v;
}

// One wavefront per chunk: cfhip_lz_parse_kernel with a record.  bytes: the slice's first TARGET byte.
__global__ __launch_bounds__(64) void cfhip_deflate_parse_kernel(const uint8_t* __restrict__ bytes, uint32_t* __restrict__ ld,
	uint32_t n, uint32_t* __restrict__ chist)
{
	__shared__ uint32_t s_ld[CFLZ_CHUNK];
	__shared__ uint32_t s_h[CFLZ_HIST];
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
	for (uint32_t i = lane; i < (uint32_t)CFLZ_HIST; i += 64u)
		s_h[i] = 0u;
	__syncthreads();
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
		uint32_t p = 0u;
		while (p < clen) {
			const uint32_t v = s_ld[p];
			s_ld[p] = v | CFLZ_SEEN;
			p += (v & CFLZ_TAKEN) ? (v & 0x1FFu) : 1u;
		}
	}
	__syncthreads();
	uint32_t extra = 0u, literals = 0u, matches = 0u, matched = 0u;
	for (uint32_t i = lane; i < clen; i += 64u) {
		const uint32_t v = s_ld[i];
		if (!(v & CFLZ_SEEN))
			continue;
		if (v & CFLZ_TAKEN) {
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
			const uint32_t b = bytes[base + i];
			atomicAdd(&s_h[b], 1u);
			++literals;
			s_ld[i] = CFLZ_SEEN | (b << 16);             // the record of a literal: its byte
		}
	}
	if (extra) atomicAdd(&s_h[CFLZ_EXTRA], extra);
	if (literals) atomicAdd(&s_h[CFLZ_LITERALS], literals);
	if (matches) atomicAdd(&s_h[CFLZ_MATCHES], matches);
	if (matched) atomicAdd(&s_h[CFLZ_MATCHED], matched);
	__syncthreads();
	for (uint32_t i = lane*4u; i < clen; i += 256u) {
		if (i + 4u <= clen)
			*reinterpret_cast<uint4*>(ld + base + i) = *reinterpret_cast<const uint4*>(s_ld + i);
		else
			for (uint32_t j = i; j < clen; ++j)
				ld[base + j] = s_ld[j];
	}
	uint32_t* out = chist + (size_t)blockIdx.x*CFLZ_HIST;
	for (uint32_t i = lane; i < (uint32_t)CFLZ_HIST; i += 64u)
		out[i] = s_h[i];
}

// One wavefront per chunk: adler[2 c] = sum of the bytes, adler[2 c + 1] = sum of (clen - i) byte_i, mod 65521.
__global__ __launch_bounds__(64) void cfhip_deflate_adler_kernel(const uint8_t* __restrict__ bytes, uint32_t n,
	uint32_t* __restrict__ adler)
{
	const uint32_t lane = threadIdx.x;
	const uint32_t base = blockIdx.x*CFLZ_CHUNK;
	const uint32_t clen = n - base < CFLZ_CHUNK ? n - base : CFLZ_CHUNK;
	uint32_t s1 = 0u, s2 = 0u;                                  // a lane sums 64 bytes: below 2^27
	for (uint32_t i = lane*16u; i < clen; i += 1024u) {
		if (i + 16u <= clen) {
			const uint4 v = *reinterpret_cast<const uint4*>(bytes + base + i);   // the slice's targets are 16-byte aligned
			const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for (uint32_t k = 0u; k < 16u; ++k) {
				const uint32_t b = (w[k >> 2] >> (8u*(k & 3u))) & 0xFFu;
				s1 += b;
				s2 += (clen - i - k)*b;
			}
		} else
			for (uint32_t j = i; j < clen; ++j) {
				const uint32_t b = bytes[base + j];
				s1 += b;
				s2 += (clen - j)*b;
			}
	}
	unsigned long long t1 = s1, t2 = s2;
	for (int s = 32; s; s >>= 1) {
		t1 += __shfl_xor(t1, s, 64);
		t2 += __shfl_xor(t2, s, 64);
	}
	if (lane == 0u) {
		adler[2u*blockIdx.x] = (uint32_t)(t1 % 65521ull);
		adler[2u*blockIdx.x + 1u] = (uint32_t)(t2 % 65521ull);
	}
}

// The code builder's LDS: an alphabet of at most 288 symbols.
struct DfWork {
	uint32_t c[288];       // the counts, after the rule for fewer than two used symbols
	uint32_t w[576];       // weights: the leaves in (count, symbol) order, then the internal nodes as they are made
	uint16_t sym[288];     // the leaves' symbols
	uint16_t par[576];
	uint16_t dep[576];
	uint32_t n[16];        // leaves per length; then the next code per length
};

// deflate_ref.code_lengths by one wavefront: lens[0 .. nsym) from cnt[0 .. nsym), 2 <= nsym <= 288, 2^limit >= nsym.
__device__ void df_build_lengths(const uint32_t* cnt, uint32_t nsym, uint32_t limit, uint8_t* lens, DfWork& k, uint32_t lane)
{
	uint32_t used = 0u;
	for (uint32_t i = lane; i < nsym; i += 64u) {
		const uint32_t v = cnt[i];
		k.c[i] = v;
		lens[i] = 0u;
		used += v != 0u;
	}
	used = df_wave_sum(used);
	__syncthreads();
	if (used < 2u) {
		if (lane == 0u) {
			uint32_t have = used;
			for (uint32_t i = 0u; have < 2u && i < nsym; ++i)
				if (!k.c[i]) {
					k.c[i] = 1u;
					++have;
				}
		}
		used = 2u;
		__syncthreads();
	}
	const uint32_t m = used;
	// rank by (count, symbol): every used symbol counts those before it
	for (uint32_t i = lane; i < nsym; i += 64u) {
		const uint32_t ci = k.c[i];
		if (!ci)
			continue;
		uint32_t r = 0u;
		for (uint32_t j = 0u; j < nsym; ++j) {
			const uint32_t cj = k.c[j];
			r += (cj != 0u && (cj < ci || (cj == ci && j < i))) ? 1u : 0u;
		}
		k.sym[r] = (uint16_t)i;
		k.w[r] = ci;
	}
	__syncthreads();
	if (lane == 0u) {
		uint32_t leaf = 0u, node = m;
		for (uint32_t t = 0u; t + 1u < m; ++t) {
			uint32_t a, b;
			if (leaf < m && (node >= m + t || k.w[leaf] <= k.w[node])) a = leaf++; else a = node++;
			if (leaf < m && (node >= m + t || k.w[leaf] <= k.w[node])) b = leaf++; else b = node++;
			k.w[m + t] = k.w[a] + k.w[b];
			k.par[a] = k.par[b] = (uint16_t)(m + t);
		}
		for (uint32_t l = 0u; l < 16u; ++l)
			k.n[l] = 0u;
		k.dep[2u*m - 2u] = 0u;
		for (uint32_t j = 2u*m - 2u; j-- > 0u;) {
			const uint32_t d = k.dep[k.par[j]] + 1u;
			k.dep[j] = (uint16_t)d;
			if (j < m)
				k.n[d < limit ? d : limit] += 1u;
		}
		uint32_t kraft = 0u;
		for (uint32_t l = 1u; l <= limit; ++l)
			kraft += k.n[l] << (limit - l);
		// (each step lowers the sum by one; it exceeds 1 by less than the number of leaves)
		for (uint32_t step = 0u; kraft > (1u << limit) && step < m; ++step) {
			uint32_t l = limit - 1u;
			while (l > 1u && !k.n[l])
				--l;
			k.n[l] -= 1u;
			k.n[l + 1u] += 2u;
			k.n[limit] -= 1u;
			--kraft;
		}
		uint32_t at = 0u;
		for (uint32_t l = limit; l; --l)
			for (uint32_t t = k.n[l]; t; --t)
				lens[k.sym[at++]] = (uint8_t)l;
	}
	__syncthreads();
}

// canonical codes (RFC 1951, 3.2.2) by lane 0: codes[i] = the bit-reversed code | length << 16
__device__ void df_build_codes(const uint8_t* lens, uint32_t nsym, uint32_t* codes, DfWork& k, uint32_t lane)
{
	if (lane == 0u) {
		for (uint32_t l = 0u; l < 16u; ++l)
			k.n[l] = 0u;
		for (uint32_t i = 0u; i < nsym; ++i)
			k.n[lens[i]] += 1u;
		uint32_t code = 0u, prev = 0u;
		for (uint32_t l = 1u; l < 16u; ++l) {
			code = (code + prev) << 1;
			prev = k.n[l];
			k.n[l] = code;
		}
		for (uint32_t i = 0u; i < nsym; ++i) {
			const uint32_t l = lens[i];
			uint32_t e = 0u;
			if (l) {
				const uint32_t c = k.n[l]++;
				e = (__brev(c) >> (32u - l)) | (l << 16);
			}
			codes[i] = e;
		}
	}
	__syncthreads();
}

// RFC 1951's fixed code of literal/length symbol i < 286
__device__ __forceinline__ uint32_t df_fixed_ll(uint32_t i)
{
	uint32_t l, c;
	if (i < 144u) { l = 8u; c = 0x30u + i; }
	else if (i < 256u) { l = 9u; c = 0x190u + (i - 144u); }
	else if (i < 280u) { l = 7u; c = i - 256u; }
	else { l = 8u; c = 0xC0u + (i - 280u); }
	return (__brev(c) >> (32u - l)) | (l << 16);
}

struct DfBits {
	unsigned long long acc;
	uint32_t nb, w;
};

__device__ __forceinline__ void df_hdr_put(uint32_t* hdr, DfBits& s, uint32_t v, uint32_t len)
{
	s.acc |= (unsigned long long)v << s.nb;
	s.nb += len;
	if (s.nb >= 32u) {
		hdr[s.w++] = (uint32_t)s.acc;
		s.acc >>= 32;
		s.nb -= 32u;
	}
}

// One wavefront per group.
__global__ __launch_bounds__(64) void cfhip_deflate_codes_kernel(const uint32_t* __restrict__ chist, uint32_t n,
	uint32_t* __restrict__ blk, uint32_t* __restrict__ tab, uint32_t* __restrict__ hdr)
{
	__shared__ DfWork k;
	__shared__ uint32_t s_cnt[CFLZ_HIST];
	__shared__ uint32_t s_code[CFDF_TAB];
	__shared__ uint32_t s_hdr[CFDF_HDR_WORDS];
	__shared__ uint32_t s_cl[20], s_clcode[20];
	__shared__ uint16_t s_tok[CFDF_TAB];
	__shared__ uint8_t s_len[CFDF_TAB + 4];
	__shared__ uint8_t s_cllen[20];
	__shared__ uint32_t s_misc[4];                   // tokens, header bits
	const uint32_t lane = threadIdx.x, b = blockIdx.x;
	const uint32_t blen = n - b*CFLZ_COSTBLK < CFLZ_COSTBLK ? n - b*CFLZ_COSTBLK : CFLZ_COSTBLK;
	const uint32_t nch = (blen + CFLZ_CHUNK - 1u)/CFLZ_CHUNK;
	const uint32_t* ch = chist + (size_t)b*CFDF_CHUNKS*CFLZ_HIST;
	for (uint32_t i = lane; i < (uint32_t)CFLZ_HIST; i += 64u) {
		uint32_t v = i == 256u ? 1u : 0u;            // the end-of-block symbol
		for (uint32_t c = 0u; c < nch; ++c)
			v += ch[c*CFLZ_HIST + i];
		s_cnt[i] = v;
	}
	for (uint32_t i = lane; i < (uint32_t)CFDF_HDR_WORDS; i += 64u)
		s_hdr[i] = 0u;
	if (lane < 20u)
		s_cl[lane] = 0u;
	__syncthreads();
	df_build_lengths(s_cnt, CFLZ_LL, CFDF_LIMIT, s_len, k, lane);
	df_build_lengths(s_cnt + CFLZ_LL, CFLZ_DD, CFDF_LIMIT, s_len + CFLZ_LL, k, lane);
	df_build_codes(s_len, CFLZ_LL, s_code, k, lane);
	df_build_codes(s_len + CFLZ_LL, CFLZ_DD, s_code + CFLZ_LL, k, lane);
	// the header's run-length tokens over the one sequence of both alphabets' lengths (deflate_ref.header_tokens)
	if (lane == 0u) {
		uint32_t hlit = CFLZ_LL, hdist = CFLZ_DD;
		while (hlit > 257u && !s_len[hlit - 1u]) --hlit;
		while (hdist > 1u && !s_len[CFLZ_LL + hdist - 1u]) --hdist;
		const uint32_t total = hlit + hdist;
		uint32_t i = 0u, ntok = 0u, before = 0xFFu;
		while (i < total) {
			const uint32_t v = s_len[i < hlit ? i : CFLZ_LL + (i - hlit)];
			uint32_t run = 1u;
			while (i + run < total && s_len[i + run < hlit ? i + run : CFLZ_LL + (i + run - hlit)] == v)
				++run;
			i += run;
			// the whole run: `before` is the entry in front of what is left of it
			for (uint32_t r = run; r;) {
				uint32_t sym = v, ev = 0u, c = 1u;
				if (v == 0u && r >= 3u) {
					c = r < 138u ? r : 138u;
					if (c >= 11u) { sym = 18u; ev = c - 11u; } else { sym = 17u; ev = c - 3u; }
				} else if (v != 0u && r >= 3u && before == v) {
					c = r < 6u ? r : 6u;
					sym = 16u;
					ev = c - 3u;
				}
				s_tok[ntok++] = (uint16_t)(sym | (ev << 5));
				s_cl[sym] += 1u;
				before = v;
				r -= c;
			}
		}
		s_misc[0] = ntok;
		s_misc[2] = hlit;
		s_misc[3] = hdist;
	}
	__syncthreads();
	df_build_lengths(s_cl, 19u, CFDF_CL_LIMIT, s_cllen, k, lane);
	df_build_codes(s_cllen, 19u, s_clcode, k, lane);
	if (lane == 0u) {
		const uint32_t ntok = s_misc[0], hlit = s_misc[2], hdist = s_misc[3];
		uint32_t hclen = 19u;
		while (hclen > 4u && !s_cllen[df_cl_order[hclen - 1u]]) --hclen;
		DfBits s = {0ull, 0u, 0u};
		df_hdr_put(s_hdr, s, 4u, 3u);                            // BFINAL 0, BTYPE 10
		df_hdr_put(s_hdr, s, hlit - 257u, 5u);
		df_hdr_put(s_hdr, s, hdist - 1u, 5u);
		df_hdr_put(s_hdr, s, hclen - 4u, 4u);
		for (uint32_t i = 0u; i < hclen; ++i)
			df_hdr_put(s_hdr, s, s_cllen[df_cl_order[i]], 3u);
		for (uint32_t i = 0u; i < ntok; ++i) {
			const uint32_t t = s_tok[i], sym = t & 31u, e = s_clcode[sym], l = e >> 16;
			const uint32_t eb = sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u;
			df_hdr_put(s_hdr, s, (e & 0xFFFFu) | ((t >> 5) << l), l + eb);
		}
		s_misc[1] = 32u*s.w + s.nb;
		if (s.nb)
			s_hdr[s.w] = (uint32_t)s.acc;
	}
	__syncthreads();
	// the exact bits of the fixed and the dynamic form, and the bytes of all three
	uint32_t fix = 0u, dyn = 0u;
	for (uint32_t i = lane; i < (uint32_t)CFDF_TAB; i += 64u) {
		const uint32_t c = s_cnt[i];
		fix += c*(i < (uint32_t)CFLZ_LL ? df_fixed_ll(i) >> 16 : 5u);
		dyn += c*s_len[i];
	}
	const uint32_t extra = s_cnt[CFLZ_EXTRA], hdr_bits = s_misc[1];
	fix = df_wave_sum(fix) + extra + 3u;
	dyn = df_wave_sum(dyn) + extra + hdr_bits;
	const uint32_t stored_sz = blen + 5u*(1u + (blen > CFDF_STORED_SPLIT ? 1u : 0u));
	const uint32_t fix_sz = (fix + 3u + 7u)/8u + 4u, dyn_sz = (dyn + 3u + 7u)/8u + 4u;
	uint32_t form = 0u, size = stored_sz;
	if (fix_sz < size) { form = 1u; size = fix_sz; }
	if (dyn_sz < size) { form = 2u; size = dyn_sz; }
	uint32_t* rec = blk + (size_t)b*CFDF_B_WORDS;
	if (form) {
		uint32_t* t = tab + (size_t)b*CFDF_TAB;
		for (uint32_t i = lane; i < (uint32_t)CFDF_TAB; i += 64u)
			t[i] = form == 2u ? s_code[i] : i < (uint32_t)CFLZ_LL ? df_fixed_ll(i) : (__brev(i - CFLZ_LL) >> 27) | (5u << 16);
		uint32_t* h = hdr + (size_t)b*CFDF_HDR_WORDS;
		for (uint32_t i = lane; i < (uint32_t)CFDF_HDR_WORDS; i += 64u)
			h[i] = form == 2u ? s_hdr[i] : i == 0u ? 2u : 0u;        // fixed: BFINAL 0, BTYPE 01
		// where each chunk's tokens start: the header, then the bits of the chunks before it
		uint32_t at = form == 2u ? hdr_bits : 3u;
		for (uint32_t c = 0u; c < nch; ++c) {
			uint32_t bits = 0u;
			for (uint32_t i = lane; i < (uint32_t)CFDF_TAB; i += 64u) {
				const uint32_t l = form == 2u ? s_len[i] : i < (uint32_t)CFLZ_LL ? df_fixed_ll(i) >> 16 : 5u;
				bits += ch[c*CFLZ_HIST + i]*l;
			}
			bits = df_wave_sum(bits) + ch[c*CFLZ_HIST + CFLZ_EXTRA];
			if (lane == 0u)
				rec[CFDF_B_CHUNK_BIT + c] = at;
			at += bits;
		}
	}
	if (lane == 0u) {
		rec[CFDF_B_FORM] = form;
		rec[CFDF_B_BYTES] = size;
		rec[CFDF_B_HDR_BITS] = form == 2u ? hdr_bits : 3u;
		rec[CFDF_B_LITERALS] = s_cnt[CFLZ_LITERALS];
		rec[CFDF_B_MATCHES] = s_cnt[CFLZ_MATCHES];
		rec[CFDF_B_MATCHED] = s_cnt[CFLZ_MATCHED];
	}
}

// The code builder alone (cfhip_deflate_code_lengths).
__global__ __launch_bounds__(64) void cfhip_deflate_lengths_kernel(const uint32_t* __restrict__ counts, uint32_t n,
	uint32_t limit, uint8_t* __restrict__ lengths)
{
	__shared__ DfWork k;
	__shared__ uint32_t s_cnt[288];
	__shared__ uint8_t s_len[288];
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = lane; i < n; i += 64u)
		s_cnt[i] = counts[i];
	__syncthreads();
	df_build_lengths(s_cnt, n, limit, s_len, k, lane);
	for (uint32_t i = lane; i < n; i += 64u)
		lengths[i] = s_len[i];
}

// One wavefront: the groups' offsets behind the running one, and the state.
__global__ __launch_bounds__(64) void cfhip_deflate_offsets_kernel(uint32_t* __restrict__ blk, uint32_t blocks,
	const uint32_t* __restrict__ adler, uint32_t n, int first, unsigned long long* __restrict__ state)
{
	__shared__ uint32_t s_a[64], s_b[64], s_l[64];
	const uint32_t lane = threadIdx.x;
	unsigned long long off = first ? 2ull : state[CFDF_S_OFF];
	uint32_t forms[3] = {0u, 0u, 0u};
	unsigned long long lit = 0ull, mat = 0ull, mby = 0ull;
	for (uint32_t b0 = 0u; b0 < blocks; b0 += 64u) {
		const uint32_t b = b0 + lane;
		uint32_t* rec = blk + (size_t)b*CFDF_B_WORDS;
		const uint32_t size = b < blocks ? rec[CFDF_B_BYTES] : 0u;
		const uint32_t incl = df_wave_scan(size, lane);
		if (b < blocks) {
			rec[CFDF_B_OFF] = (uint32_t)(off + incl - size);
			const uint32_t f = rec[CFDF_B_FORM];
			forms[0] += f == 0u;
			forms[1] += f == 1u;
			forms[2] += f == 2u;
			lit += rec[CFDF_B_LITERALS];
			mat += rec[CFDF_B_MATCHES];
			mby += rec[CFDF_B_MATCHED];
		}
		off += __shfl(incl, 63, 64);
	}
	for (int s = 32; s; s >>= 1) {
		lit += __shfl_xor(lit, s, 64);
		mat += __shfl_xor(mat, s, 64);
		mby += __shfl_xor(mby, s, 64);
	}
	const uint32_t f0 = df_wave_sum(forms[0]), f1 = df_wave_sum(forms[1]), f2 = df_wave_sum(forms[2]);
	// Adler-32: a lane folds a run of chunks, lane 0 folds the lanes behind the state
	const uint32_t chunks = (n + CFLZ_CHUNK - 1u)/CFLZ_CHUNK, per = (chunks + 63u)/64u;
	const uint32_t c0 = lane*per < chunks ? lane*per : chunks, c1 = c0 + per < chunks ? c0 + per : chunks;
	unsigned long long A = 0ull, B = 0ull, L = 0ull;
	for (uint32_t c = c0; c < c1; ++c) {
		const uint32_t len = n - c*CFLZ_CHUNK < CFLZ_CHUNK ? n - c*CFLZ_CHUNK : CFLZ_CHUNK;
		B = (B + len*A + adler[2u*c + 1u]) % 65521ull;
		A = (A + adler[2u*c]) % 65521ull;
		L = (L + len) % 65521ull;
	}
	s_a[lane] = (uint32_t)A;
	s_b[lane] = (uint32_t)B;
	s_l[lane] = (uint32_t)L;
	__syncthreads();
	if (lane == 0u) {
		A = first ? 0ull : state[CFDF_S_A];
		B = first ? 0ull : state[CFDF_S_B];
		L = first ? 0ull : state[CFDF_S_LEN];
		for (uint32_t i = 0u; i < 64u; ++i) {
			B = (B + (unsigned long long)s_l[i]*A + s_b[i]) % 65521ull;
			A = (A + s_a[i]) % 65521ull;
			L = (L + s_l[i]) % 65521ull;
		}
		state[CFDF_S_OFF] = off;
		state[CFDF_S_A] = A;
		state[CFDF_S_B] = B;
		state[CFDF_S_LEN] = L;
		state[CFDF_S_STORED] = (first ? 0ull : state[CFDF_S_STORED]) + f0;
		state[CFDF_S_STORED + 1] = (first ? 0ull : state[CFDF_S_STORED + 1]) + f1;
		state[CFDF_S_STORED + 2] = (first ? 0ull : state[CFDF_S_STORED + 2]) + f2;
		state[CFDF_S_LITERALS] = (first ? 0ull : state[CFDF_S_LITERALS]) + lit;
		state[CFDF_S_MATCHES] = (first ? 0ull : state[CFDF_S_MATCHES]) + mat;
		state[CFDF_S_MATCHED] = (first ? 0ull : state[CFDF_S_MATCHED]) + mby;
	}
}

// at most `len` <= 32 bits of v at bit `pos` of the zeroed LDS words
__device__ __forceinline__ void df_put(uint32_t* buf, uint32_t pos, uint32_t v)
{
	const unsigned long long x = (unsigned long long)v << (pos & 31u);
	const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
	if (lo) atomicOr(&buf[pos >> 5], lo);
	if (hi) atomicOr(&buf[(pos >> 5) + 1u], hi);
}

// The words of one chunk's bits: 4096 literals of 15 bits, in front of them a header (chunk 0) and up to 31 bits of
// the word they start in, behind them the end-of-block code and the closing block: 61440 + 2286 + 31 + 15 + 42 bits.
#define DF_OUT_WORDS 2000
// the staged words are padded by one per 64: a lane reads 64 consecutive positions, each lane in another bank
#define DF_PAD(i) ((i) + ((i) >> 6))

// One wavefront per chunk.  bytes: the slice's first TARGET byte.
__global__ __launch_bounds__(64) void cfhip_deflate_emit_kernel(const uint8_t* __restrict__ bytes,
	const uint32_t* __restrict__ ld, uint32_t n, const uint32_t* __restrict__ blk, const uint32_t* __restrict__ tab,
	const uint32_t* __restrict__ hdr, int last, uint32_t* __restrict__ out)
{
	__shared__ uint32_t s_ld[CFLZ_CHUNK + CFLZ_CHUNK/64u];
	__shared__ uint32_t s_tab[CFDF_TAB];
	__shared__ uint32_t s_out[DF_OUT_WORDS];
	const uint32_t lane = threadIdx.x;
	const uint32_t base = blockIdx.x*CFLZ_CHUNK;
	const uint32_t clen = n - base < CFLZ_CHUNK ? n - base : CFLZ_CHUNK;
	const uint32_t b = blockIdx.x/CFDF_CHUNKS, c = blockIdx.x % CFDF_CHUNKS;
	const uint32_t blen = n - b*CFLZ_COSTBLK < CFLZ_COSTBLK ? n - b*CFLZ_COSTBLK : CFLZ_COSTBLK;
	const uint32_t nch = (blen + CFLZ_CHUNK - 1u)/CFLZ_CHUNK;
	const uint32_t* rec = blk + (size_t)b*CFDF_B_WORDS;
	const uint32_t form = rec[CFDF_B_FORM], off = rec[CFDF_B_OFF];
	const bool final_group = last && b == (n - 1u)/CFLZ_COSTBLK;
	if (form == 0u) {
		// stored: one block per 32768 bytes, its five header bytes in front of chunks 0 and 8
		const uint32_t sub = c >= 8u ? 1u : 0u;
		if ((c & 7u) == 0u && lane < 5u) {
			const uint32_t rest = blen - sub*CFDF_STORED_SPLIT;
			const uint32_t slen = rest < CFDF_STORED_SPLIT ? rest : CFDF_STORED_SPLIT;
			const uint32_t fin = final_group && sub*CFDF_STORED_SPLIT + slen == blen ? 1u : 0u;
			const uint32_t at = off + sub*(CFDF_STORED_SPLIT + 5u) + lane;
			const uint32_t v = lane == 0u ? fin : lane == 1u ? slen & 0xFFu : lane == 2u ? (slen >> 8) & 0xFFu :
				lane == 3u ? ~slen & 0xFFu : (~slen >> 8) & 0xFFu;
			if (v)
				atomicOr(out + (at >> 2), v << (8u*(at & 3u)));
		}
		const unsigned long long dst = (unsigned long long)off + 5u*(1u + sub) + base - b*CFLZ_COSTBLK;
		const uint8_t* src = bytes + base;
		const unsigned long long w0 = dst >> 2, w1 = (dst + clen - 1u) >> 2;
		for (unsigned long long w = w0 + lane; w <= w1; w += 64u) {
			const long long j = (long long)(4ull*w) - (long long)dst;        // the source byte of the word's byte 0
			if (j >= 0 && j + 4 <= (long long)clen)
				out[w] = df_load32(src + j);
			else {
				uint32_t v = 0u;
				for (int q = 0; q < 4; ++q)
					if (j + q >= 0 && j + q < (long long)clen)
						v |= (uint32_t)src[j + q] << (8*q);
				if (v)
					atomicOr(out + w, v);
			}
		}
		return;
	}
	for (uint32_t i = lane*4u; i < CFLZ_CHUNK; i += 256u) {
		uint4 v = make_uint4(0u, 0u, 0u, 0u);
		if (i + 4u <= clen)
			v = *reinterpret_cast<const uint4*>(ld + base + i);
		else {
			if (i < clen) v.x = ld[base + i];
			if (i + 1u < clen) v.y = ld[base + i + 1u];
			if (i + 2u < clen) v.z = ld[base + i + 2u];
		}
		uint32_t* d = s_ld + DF_PAD(i);
		d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
	}
	for (uint32_t i = lane; i < (uint32_t)CFDF_TAB; i += 64u)
		s_tab[i] = tab[(size_t)b*CFDF_TAB + i];
	for (uint32_t i = lane; i < (uint32_t)DF_OUT_WORDS; i += 64u)
		s_out[i] = 0u;
	__syncthreads();
	// a lane owns the 64 positions from 64 lane on: its tokens' bits, then where they start
	const uint32_t* row = s_ld + 65u*lane;
	uint32_t bits = 0u;
	for (uint32_t t = 0u; t < 64u; ++t) {
		const uint32_t v = row[t];
		if (!(v & CFLZ_SEEN))
			continue;
		if (v & CFLZ_TAKEN) {
			uint32_t el, ed;
			const uint32_t lc = lz_length_code(v & 0x1FFu, &el);
			const uint32_t dc = lz_dist_code(v >> 16, &ed);
			bits += (s_tab[257u + lc] >> 16) + el + (s_tab[(uint32_t)CFLZ_LL + dc] >> 16) + ed;
		} else
			bits += s_tab[(v >> 16) & 0xFFu] >> 16;
	}
	const uint32_t incl = df_wave_scan(bits, lane);
	const uint32_t total = __shfl(incl, 63, 64);
	const uint32_t hdr_bits = c ? 0u : rec[CFDF_B_HDR_BITS];
	const unsigned long long gbit = 8ull*off + (c ? rec[CFDF_B_CHUNK_BIT + c] : 0u);
	const unsigned long long word0 = gbit >> 5;
	const uint32_t sh = (uint32_t)gbit & 31u;
	if (c == 0u)
		for (uint32_t w = lane; w < (hdr_bits + 31u)/32u; w += 64u)
			df_put(s_out, sh + 32u*w, hdr[(size_t)b*CFDF_HDR_WORDS + w]);
	uint32_t pos = sh + hdr_bits + incl - bits;
	for (uint32_t t = 0u; t < 64u; ++t) {
		const uint32_t v = row[t];
		if (!(v & CFLZ_SEEN))
			continue;
		if (v & CFLZ_TAKEN) {
			uint32_t el, ed;
			const uint32_t len = v & 0x1FFu, d1 = v >> 16;
			const uint32_t lc = lz_length_code(len, &el);
			const uint32_t dc = lz_dist_code(d1, &ed);
			const uint32_t le = s_tab[257u + lc], de = s_tab[(uint32_t)CFLZ_LL + dc];
			df_put(s_out, pos, (le & 0xFFFFu) | (((len - 3u) & ((1u << el) - 1u)) << (le >> 16)));
			pos += (le >> 16) + el;
			df_put(s_out, pos, (de & 0xFFFFu) | ((d1 & ((1u << ed) - 1u)) << (de >> 16)));
			pos += (de >> 16) + ed;
		} else {
			const uint32_t e = s_tab[(v >> 16) & 0xFFu];
			df_put(s_out, pos, e & 0xFFFFu);
			pos += e >> 16;
		}
	}
	// the group's last chunk ends it: the end-of-block code and the closing block (an empty stored block)
	uint32_t end = sh + hdr_bits + total;
	if (c == nch - 1u) {
		const uint32_t e = s_tab[256];
		if (lane == 0u)
			df_put(s_out, end, e & 0xFFFFu);
		end += e >> 16;
		if (lane == 0u && final_group)
			df_put(s_out, end, 1u);
		end = (end + 3u + 7u) & ~7u;
		if (lane == 0u)
			df_put(s_out, end, 0xFFFF0000u);
		end += 32u;
	}
	__syncthreads();
	const uint32_t nw = (end + 31u) >> 5;
	for (uint32_t w = lane; w < nw; w += 64u) {
		const uint32_t v = s_out[w];
		if (w == 0u || w == nw - 1u) {
			if (v)
				atomicOr(out + word0 + w, v);
		} else
			out[word0 + w] = v;
	}
}

__global__ void cfhip_deflate_final_kernel(const unsigned long long* __restrict__ state, unsigned long long bytes_in,
	uint8_t* __restrict__ out, unsigned long long* __restrict__ result)
{
	if (threadIdx.x || blockIdx.x)
		return;
	const unsigned long long off = state[CFDF_S_OFF];
	const uint32_t a = (uint32_t)((1ull + state[CFDF_S_A]) % 65521ull);
	const uint32_t b = (uint32_t)((state[CFDF_S_B] + state[CFDF_S_LEN]) % 65521ull);   // the leading 1, once per byte
	const uint32_t adler = (b << 16) | a;
	out[0] = 0x78u;
	out[1] = 0x9Cu;
	out[off] = (uint8_t)(adler >> 24);
	out[off + 1u] = (uint8_t)(adler >> 16);
	out[off + 2u] = (uint8_t)(adler >> 8);
	out[off + 3u] = (uint8_t)adler;
	result[0] = bytes_in;
	result[1] = off + 4ull;
	result[2] = state[CFDF_S_STORED];
	result[3] = state[CFDF_S_STORED + 1];
	result[4] = state[CFDF_S_STORED + 2];
	result[5] = state[CFDF_S_LITERALS];
	result[6] = state[CFDF_S_MATCHES];
	result[7] = state[CFDF_S_MATCHED];
	result[8] = adler;                                           // adler32, then reserved = 0
}

} // namespace

extern "C" hipError_t cfhip_launch_deflate_slice(uint8_t* base, const cfdf_layout* lay, size_t sort_bytes, uint32_t carry,
	uint32_t n, int first, int last, uint8_t* out, hipEvent_t* ev, hipStream_t stream)
{
	const uint32_t blocks = (n + CFLZ_COSTBLK - 1u)/CFLZ_COSTBLK, chunks = (n + CFLZ_CHUNK - 1u)/CFLZ_CHUNK;
	const uint8_t* bytes = base + lay->lz.bytes + carry;
	uint32_t* ld = reinterpret_cast<uint32_t*>(base + lay->lz.ld);
	uint32_t* chist = reinterpret_cast<uint32_t*>(base + lay->chist);
	uint32_t* adler = reinterpret_cast<uint32_t*>(base + lay->adler);
	uint32_t* blk = reinterpret_cast<uint32_t*>(base + lay->blk);
	uint32_t* tab = reinterpret_cast<uint32_t*>(base + lay->tab);
	uint32_t* hdr = reinterpret_cast<uint32_t*>(base + lay->hdr);
	unsigned long long* state = reinterpret_cast<unsigned long long*>(base + lay->state);
	hipError_t e = cfhip_launch_lz_matches(base, &lay->lz, sort_bytes, carry, n, ev, stream);
	if (e != hipSuccess)
		return e;
#define DF_STAGE(k, ...) do { \
		if (ev && (e = hipEventRecord(ev[2*(k)], stream)) != hipSuccess) return e; \
		hipLaunchKernelGGL(__VA_ARGS__); \
		if ((e = hipGetLastError()) != hipSuccess) return e; \
		if (ev && (e = hipEventRecord(ev[2*(k) + 1], stream)) != hipSuccess) return e; \
	} while (0)
	DF_STAGE(3, cfhip_deflate_parse_kernel, dim3(chunks), dim3(64), 0, stream, bytes, ld, n, chist);
	DF_STAGE(4, cfhip_deflate_adler_kernel, dim3(chunks), dim3(64), 0, stream, bytes, n, adler);
	DF_STAGE(5, cfhip_deflate_codes_kernel, dim3(blocks), dim3(64), 0, stream, chist, n, blk, tab, hdr);
	DF_STAGE(6, cfhip_deflate_offsets_kernel, dim3(1), dim3(64), 0, stream, blk, blocks, adler, n, first, state);
	DF_STAGE(7, cfhip_deflate_emit_kernel, dim3(chunks), dim3(64), 0, stream, bytes, ld, n, blk, tab, hdr, last,
		reinterpret_cast<uint32_t*>(out));
#undef DF_STAGE
	return hipSuccess;
}

extern "C" hipError_t cfhip_launch_deflate_final(const unsigned long long* state, unsigned long long bytes_in, uint8_t* out,
	unsigned long long* result, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_deflate_final_kernel, dim3(1), dim3(64), 0, stream, state, bytes_in, out, result);
	return hipGetLastError();
}

extern "C" hipError_t cfhip_launch_deflate_code_lengths(const uint32_t* counts, uint32_t n, uint32_t limit,
	uint8_t* lengths, hipStream_t stream)
{
	hipLaunchKernelGGL(cfhip_deflate_lengths_kernel, dim3(1), dim3(64), 0, stream, counts, n, limit, lengths);
	return hipGetLastError();
}
