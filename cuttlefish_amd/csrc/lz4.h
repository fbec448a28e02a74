// lz4.h -- what the host side (cfhip_api.hip), the kernels (lz4.hip) and the host program (tools/lz4_host.cpp) of the LZ4
// frame codec share: the constants of the format, XXH32, the functions that parse and check a frame -- its header, its
// block chain, one sequence -- and, for the device side, the scratch layouts and the launchers.
// The definition of every byte and every verdict is tests/lz4_ref.py; every constant below has
// its twin there.  Everything above the __HIPCC__ part compiles with the host compiler alone.
#ifndef CF_LZ4_H
#define CF_LZ4_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CFLZ4_FN __host__ __device__ inline
#else
#define CFLZ4_FN inline
#endif

#define CFLZ4_BLOCK 65536u          // input bytes per block: BD code 4
#define CFLZ4_HEADER 15u            // magic, FLG, BD, content size, HC
#define CFLZ4_FLG 0x78u             // version 01, independent blocks, block checksums, content size
#define CFLZ4_BD 0x40u
#define CFLZ4_LAST_LITERALS 5u      // the last bytes of a block are literals
#define CFLZ4_MATCH_MARGIN 12u      // no match starts later than this before the block's end
#define CFLZ4_RAW 0x80000000u       // bit 31 of a block's size word: stored raw

// The classes of cfhip_lz4_decode_result.status (tests/lz4_ref.py states which defect yields which, and in what order).
#define CFLZ4_OK 0u
#define CFLZ4_E_HEADER 1u
#define CFLZ4_E_UNSUPPORTED 2u
#define CFLZ4_E_BLOCKS 3u
#define CFLZ4_E_CHECKSUM 4u
#define CFLZ4_E_SEQUENCE 5u
#define CFLZ4_E_OFFSET 6u
#define CFLZ4_E_SIZE 7u

// The timed stages, in launch order.
#define CFLZ4_STAGES 9              // encode: keys, sort, match, parse, plan, offsets, emit, hash, final
#define CFLZ4_DSTAGES 3             // decode: chain, blocks, final

inline size_t cflz4_bound(size_t n)
{
	return 19u + n + 8u*((n + CFLZ4_BLOCK - 1u)/CFLZ4_BLOCK);
}

// ---- XXH32 ---------------------------------------------------------------------------------------------------------
#define CFLZ4_P1 2654435761u
#define CFLZ4_P2 2246822519u
#define CFLZ4_P3 3266489917u
#define CFLZ4_P4 668265263u
#define CFLZ4_P5 374761393u

CFLZ4_FN uint32_t cflz4_rotl(uint32_t x, uint32_t r)
{
	return (x << r) | (x >> (32u - r));
}

CFLZ4_FN uint32_t cflz4_le32(const uint8_t* p)
{
	return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// one of the four accumulators over one word of a 16-byte stripe
CFLZ4_FN uint32_t cflz4_xxh_round(uint32_t acc, uint32_t w)
{
	return cflz4_rotl(acc + w*CFLZ4_P2, 13u)*CFLZ4_P1;
}

// accumulator i's start at seed 0
CFLZ4_FN uint32_t cflz4_xxh_init(uint32_t i)
{
	return i == 0u ? CFLZ4_P1 + CFLZ4_P2 : i == 1u ? CFLZ4_P2 : i == 2u ? 0u : 0u - CFLZ4_P1;
}

CFLZ4_FN uint32_t cflz4_xxh_merge(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3)
{
	return cflz4_rotl(v0, 1u) + cflz4_rotl(v1, 7u) + cflz4_rotl(v2, 12u) + cflz4_rotl(v3, 18u);
}

// h: the merged accumulators (n >= 16) or CFLZ4_P5 (n < 16); tail: the n & 15 bytes behind the last whole stripe
CFLZ4_FN uint32_t cflz4_xxh_finish(uint32_t h, const uint8_t* tail, uint32_t n)
{
	uint32_t left = n & 15u;
	h += n;
	for (; left >= 4u; left -= 4u, tail += 4)
		h = cflz4_rotl(h + cflz4_le32(tail)*CFLZ4_P3, 17u)*CFLZ4_P4;
	for (; left; --left, ++tail)
		h = cflz4_rotl(h + (uint32_t)tail[0]*CFLZ4_P5, 11u)*CFLZ4_P1;
	h ^= h >> 15;
	h *= CFLZ4_P2;
	h ^= h >> 13;
	h *= CFLZ4_P3;
	return h ^ (h >> 16);
}

// XXH32(p[0 .. n), seed 0), one lane wide
CFLZ4_FN uint32_t cflz4_xxh32(const uint8_t* p, uint32_t n)
{
	uint32_t h = CFLZ4_P5;
	const uint32_t stripes = n >> 4;
	if (stripes) {
		uint32_t v0 = cflz4_xxh_init(0u), v1 = cflz4_xxh_init(1u), v2 = cflz4_xxh_init(2u), v3 = cflz4_xxh_init(3u);
		for (uint32_t s = 0u; s < stripes; ++s, p += 16) {
			v0 = cflz4_xxh_round(v0, cflz4_le32(p));
			v1 = cflz4_xxh_round(v1, cflz4_le32(p + 4));
			v2 = cflz4_xxh_round(v2, cflz4_le32(p + 8));
			v3 = cflz4_xxh_round(v3, cflz4_le32(p + 12));
		}
		h = cflz4_xxh_merge(v0, v1, v2, v3);
	}
	return cflz4_xxh_finish(h, p, n);
}

// ---- the frame header ------------------------------------------------------------------------------------------------
struct cflz4_header {
	uint32_t length;            // bytes in front of the first block
	uint32_t block_checksums;   // 0 / 1: four bytes behind every block
	uint32_t content_checksum;  // 0 / 1: four bytes behind the end mark (not verified)
};

// The header of the 15 bytes cfhip_lz4_encode writes for n input bytes.
CFLZ4_FN void cflz4_write_header(uint8_t* out, uint64_t n)
{
	out[0] = 0x04u; out[1] = 0x22u; out[2] = 0x4Du; out[3] = 0x18u;
	out[4] = (uint8_t)CFLZ4_FLG;
	out[5] = (uint8_t)CFLZ4_BD;
	for (uint32_t i = 0u; i < 8u; ++i)
		out[6u + i] = (uint8_t)(n >> (8u*i));
	out[14] = (uint8_t)(cflz4_xxh32(out + 4, 10u) >> 8);
}

// z[0 .. bytes): reads nothing behind it.  -> a class; *h is valid for CFLZ4_OK.
CFLZ4_FN uint32_t cflz4_parse_header(const uint8_t* z, uint64_t bytes, uint64_t out_bytes, cflz4_header* h)
{
	if (bytes < 7u || z[0] != 0x04u || z[1] != 0x22u || z[2] != 0x4Du || z[3] != 0x18u)
		return CFLZ4_E_HEADER;
	const uint32_t flg = z[4], bd = z[5], code = (bd >> 4) & 7u;
	if ((flg >> 6) != 1u || (flg & 2u) || (bd & 0x8Fu) || code < 4u)
		return CFLZ4_E_HEADER;
	const uint32_t hlen = 7u + ((flg & 8u) ? 8u : 0u) + ((flg & 1u) ? 4u : 0u);
	if (bytes < hlen || z[hlen - 1u] != ((cflz4_xxh32(z + 4, hlen - 5u) >> 8) & 0xFFu))
		return CFLZ4_E_HEADER;
	if (!(flg & 0x20u) || (flg & 1u) || code != 4u)
		return CFLZ4_E_UNSUPPORTED;
	if (flg & 8u) {
		uint64_t n = 0u;
		for (uint32_t i = 0u; i < 8u; ++i)
			n |= (uint64_t)z[6u + i] << (8u*i);
		if (n != out_bytes)
			return CFLZ4_E_SIZE;
	}
	h->length = hlen;
	h->block_checksums = (flg >> 4) & 1u;
	h->content_checksum = (flg >> 2) & 1u;
	return CFLZ4_OK;
}

// ---- the block chain -------------------------------------------------------------------------------------------------
// One hop: the block whose size word lies at *pos.  -> a class; for CFLZ4_OK *at is the block's first byte, *size its
// stored bytes, *raw its form, and *pos lies behind the block (and its checksum).
CFLZ4_FN uint32_t cflz4_next_block(const uint8_t* z, uint64_t bytes, uint32_t block_checksums, uint64_t* pos, uint64_t* at,
	uint32_t* size, uint32_t* raw)
{
	if (*pos + 4u > bytes)
		return CFLZ4_E_BLOCKS;
	const uint32_t word = cflz4_le32(z + *pos);
	if (word == 0u)
		return CFLZ4_E_SIZE;                         // the end mark, early
	const uint32_t s = word & ~CFLZ4_RAW;
	if (s > CFLZ4_BLOCK || s == 0u || *pos + 4u + s + 4u*block_checksums > bytes)
		return CFLZ4_E_BLOCKS;
	*at = *pos + 4u;
	*size = s;
	*raw = word >> 31;
	*pos += 4u + s + 4u*block_checksums;
	return CFLZ4_OK;
}

// Behind the last block: the end mark, the content checksum's room, and nothing more.
CFLZ4_FN uint32_t cflz4_frame_end(const uint8_t* z, uint64_t bytes, uint32_t content_checksum, uint64_t pos)
{
	if (pos + 4u > bytes || cflz4_le32(z + pos) != 0u)
		return CFLZ4_E_BLOCKS;
	return pos + 4u + 4u*content_checksum == bytes ? CFLZ4_OK : CFLZ4_E_BLOCKS;
}

// ---- one sequence ----------------------------------------------------------------------------------------------------
struct cflz4_seq {
	uint32_t lit_at, lit_len;   // the literals: in[lit_at .. lit_at + lit_len) -> out[op ..)
	uint32_t offset, match_len; // then match_len bytes from `offset` back; match_len 0: the block's last sequence
};

// A length nibble of 15: the 255-runs behind it.  Every byte is checked against `size` before it is read.
CFLZ4_FN bool cflz4_runs(const uint8_t* in, uint32_t size, uint32_t* ip, uint32_t* v)
{
	for (;;) {
		if (*ip >= size)
			return false;
		const uint32_t b = in[(*ip)++];
		*v += b;                                     // at most 255 x 65536
		if (b != 255u)
			return true;
	}
}

// The sequence at in[*ip] of a block of `size` stored bytes that decodes to `want` bytes, *op of them written so far.
// -> a class; for CFLZ4_OK *s holds ranges that lie inside the input and the output, and *ip is advanced (to `size`
// behind the last sequence).  The caller adds lit_len and match_len to *op after copying.
CFLZ4_FN uint32_t cflz4_sequence(const uint8_t* in, uint32_t size, uint32_t want, uint32_t* ip, uint32_t op, cflz4_seq* s)
{
	if (*ip >= size)
		return CFLZ4_E_SEQUENCE;
	const uint32_t token = in[(*ip)++];
	uint32_t ll = token >> 4;
	if (ll == 15u && !cflz4_runs(in, size, ip, &ll))
		return CFLZ4_E_SEQUENCE;
	if (ll > size - *ip || ll > want - op)
		return CFLZ4_E_SEQUENCE;
	s->lit_at = *ip;
	s->lit_len = ll;
	s->offset = 0u;
	s->match_len = 0u;
	*ip += ll;
	op += ll;
	if (*ip == size)
		return CFLZ4_OK;
	if (size - *ip < 2u)
		return CFLZ4_E_SEQUENCE;
	const uint32_t off = (uint32_t)in[*ip] | (uint32_t)in[*ip + 1u] << 8;
	*ip += 2u;
	if (off == 0u || off > op)
		return CFLZ4_E_OFFSET;
	uint32_t ml = token & 15u;
	if (ml == 15u && !cflz4_runs(in, size, ip, &ml))
		return CFLZ4_E_SEQUENCE;
	ml += 4u;
	if (ml > want - op)
		return CFLZ4_E_SEQUENCE;
	s->offset = off;
	s->match_len = ml;
	return CFLZ4_OK;
}

#ifdef __HIPCC__
// ---- the device side -------------------------------------------------------------------------------------------------
#include "lzsize.h"

#define CFLZ4_CHUNKS (CFLZ4_BLOCK/CFLZ_CHUNK)          // chunks of a block
#define CFLZ4_CHUNK_MATCHES (CFLZ_CHUNK/CFLZ_MIN)      // a chunk's match list: at most one per four bytes
#define CFLZ4_BLOCK_MATCHES (CFLZ4_CHUNKS*CFLZ4_CHUNK_MATCHES)
// One block's record (uint32).
#define CFLZ4_B_SIZE 0             // bytes as stored
#define CFLZ4_B_RAW 1
#define CFLZ4_B_OFF 2              // where the block's size word lies in the frame (the offsets stage)
#define CFLZ4_B_SEQS 3             // sequences with a match
#define CFLZ4_B_TAIL 4             // where the last, literal-only sequence's literals start
#define CFLZ4_B_TAIL_OFF 5         // and where its token lies in the block's encoding
#define CFLZ4_B_MATCHED 6
#define CFLZ4_B_WORDS 8
// The state carried from slice to slice (uint64).
#define CFLZ4_S_OFF 0
#define CFLZ4_S_COMPRESSED 1
#define CFLZ4_S_STORED 2
#define CFLZ4_S_SEQS 3
#define CFLZ4_S_LITERALS 4
#define CFLZ4_S_MATCHED 5
#define CFLZ4_S_WORDS 8

// The scratch of one encoder slice: the estimator's (the match stages run on it), and behind it per chunk a list of
// merged matches (start in the block | distance << 16, length) with its count, per block the planned sequences
// (where in the encoding, first literal, match start, length | distance << 16) and a record, and the state.
struct cflz4_layout {
	cflz_layout lz;
	size_t mrec, mcount, seq, blk, state, total;
};

inline cflz4_layout cflz4_scratch(size_t slice, size_t sort_bytes)
{
	auto up = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
	const size_t chunks = slice/CFLZ_CHUNK, blocks = slice/CFLZ4_BLOCK;
	cflz4_layout l;
	l.lz = cflz_scratch(slice, sort_bytes);
	size_t o = l.lz.total;
	l.mrec = o;   o = up(o + chunks*CFLZ4_CHUNK_MATCHES*8u);
	l.mcount = o; o = up(o + chunks*4u);
	l.seq = o;    o = up(o + blocks*CFLZ4_BLOCK_MATCHES*16u);
	l.blk = o;    o = up(o + blocks*CFLZ4_B_WORDS*4u);
	l.state = o;  o = up(o + CFLZ4_S_WORDS*8u);
	l.total = o;
	return l;
}

// One encoder slice of n bytes (whole blocks but for the stream's last), no carry: base's byte array holds them.
// out: the frame's buffer.  first: the stream's first slice (the state starts).  ev: NULL or 2 x 8 events (the stages
// before `final`).
extern "C" hipError_t cfhip_launch_lz4_slice(uint8_t* base, const cflz4_layout* lay, size_t sort_bytes, uint32_t n, int first,
	uint8_t* out, hipEvent_t* ev, hipStream_t stream);

// After the last slice: the header, the end mark and the seven words of cfhip_lz4_result.  ev: NULL or one pair.
extern "C" hipError_t cfhip_launch_lz4_final(const unsigned long long* state, unsigned long long bytes_in, uint8_t* out,
	unsigned long long* result, hipEvent_t* ev, hipStream_t stream);

// The decoder's scratch: per block where its bytes lie in the frame and its size word, and the state.
#define CFLZ4_D_STATUS 0           // (block << 3 | class) of the lowest failing block, or ~0
#define CFLZ4_D_COMPRESSED 1
#define CFLZ4_D_STORED 2
#define CFLZ4_D_SEQS 3
#define CFLZ4_D_LITERALS 4
#define CFLZ4_D_MATCHED 5
#define CFLZ4_D_CHECKSUMS 6        // the header's two flags: block checksums | content checksum << 1
#define CFLZ4_D_GOOD 7             // blocks the chain walk reached
#define CFLZ4_D_WORDS 8

struct cflz4_dlayout {
	size_t rec, state, total;
};

inline cflz4_dlayout cflz4_dscratch(size_t blocks)
{
	auto up = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
	cflz4_dlayout l;
	size_t o = 0;
	l.rec = o;   o = up(o + blocks*16u);
	l.state = o; o = up(o + CFLZ4_D_WORDS*8u);
	l.total = o;
	return l;
}

// The frame z[0 .. bytes) into out[0 .. out_bytes) (4-byte aligned) and the nine words of cfhip_lz4_decode_result.
// ev: NULL or 2 x CFLZ4_DSTAGES events.
extern "C" hipError_t cfhip_launch_lz4_decode(uint8_t* base, const cflz4_dlayout* lay, const uint8_t* z, unsigned long long bytes,
	uint8_t* out, unsigned long long out_bytes, unsigned long long* result, hipEvent_t* ev, hipStream_t stream);
#endif

#endif
