// deflate.h -- what the host side (cfhip_api.hip) and the kernels (deflate.hip) of the zlib encoder share: the constants
// of the format, the layout of a slice's scratch and the launchers.
// The definition of the bytes is tests/deflate_ref.py; every constant below has its twin
// there.  The stream, its matches and its parse are the estimator's (lzsize.h, tests/lzsize_ref.py).
#ifndef CF_DEFLATE_H
#define CF_DEFLATE_H
#include "lzsize.h"

#define CFDF_STORED_SPLIT 32768u   // bytes per stored block
#define CFDF_LIMIT 15              // longest literal/length and distance code
#define CFDF_CL_LIMIT 7            // longest code-length code
#define CFDF_CHUNKS (CFLZ_COSTBLK/CFLZ_CHUNK)    // chunks of a block group
// One group's code table (uint32, bit-reversed code | length << 16): ll[286], then dd[30].
#define CFDF_TAB (CFLZ_LL + CFLZ_DD)
// One group's header bits (BFINAL, BTYPE and the code tables): at most 3 + 14 + 57 + 316 x 7 = 2286 bits.
#define CFDF_HDR_WORDS 72
// One group's record (uint32).
#define CFDF_B_FORM 0              // 0 stored, 1 fixed, 2 dynamic
#define CFDF_B_BYTES 1             // bytes of the group in the stream
#define CFDF_B_HDR_BITS 2          // header bits before the first token
#define CFDF_B_OFF 3               // where the group starts in the stream (the offsets stage)
#define CFDF_B_LITERALS 4
#define CFDF_B_MATCHES 5
#define CFDF_B_MATCHED 6
#define CFDF_B_CHUNK_BIT 8         // [CFDF_CHUNKS]: the bit, from the group's start, of each chunk's first token
#define CFDF_B_WORDS 24
// The state carried from slice to slice (uint64).
#define CFDF_S_OFF 0               // bytes of the stream so far
#define CFDF_S_A 1                 // Adler-32 sums of the bytes so far, without the leading 1, and their count mod 65521
#define CFDF_S_B 2
#define CFDF_S_LEN 3
#define CFDF_S_STORED 4            // groups per form: stored, fixed, dynamic
#define CFDF_S_LITERALS 7
#define CFDF_S_MATCHES 8
#define CFDF_S_MATCHED 9
#define CFDF_S_WORDS 16
// The eight timed stages of a slice, in launch order: the estimator's keys, sort and match, then parse (with the
// record), adler, codes, offsets, emit.
#define CFDF_STAGES 8

inline size_t cfdf_bound(size_t n)
{
	return 11u + n + 10u*((n + CFLZ_COSTBLK - 1u)/CFLZ_COSTBLK);
}

// The scratch of one slice: the estimator's (the match stages run on it unchanged) and behind it, per chunk, 320
// counters and two Adler sums; per group, a record, a code table and the header bits; the state.
struct cfdf_layout {
	cflz_layout lz;
	size_t chist, adler, blk, tab, hdr, state, total;
};

inline cfdf_layout cfdf_scratch(size_t slice, size_t sort_bytes)
{
	auto up = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
	const size_t chunks = slice/CFLZ_CHUNK, blocks = slice/CFLZ_COSTBLK;
	cfdf_layout l;
	l.lz = cflz_scratch(slice, sort_bytes);
	size_t o = l.lz.total;
	l.chist = o; o = up(o + chunks*CFLZ_HIST*4u);
	l.adler = o; o = up(o + chunks*8u);
	l.blk = o;   o = up(o + blocks*CFDF_B_WORDS*4u);
	l.tab = o;   o = up(o + blocks*CFDF_TAB*4u);
	l.hdr = o;   o = up(o + blocks*CFDF_HDR_WORDS*4u);
	l.state = o; o = up(o + CFDF_S_WORDS*8u);
	l.total = o;
	return l;
}

// One slice.  base: the scratch; its byte array holds `carry` source bytes and the n target bytes.  out: the stream's
// buffer (4-byte aligned, zeroed up to cfdf_bound before the first slice).  first / last: the stream's first / last
// slice (the state starts at the first; BFINAL goes into the last group of the last).  ev: NULL or 2 x CFDF_STAGES.
extern "C" hipError_t cfhip_launch_deflate_slice(uint8_t* base, const cfdf_layout* lay, size_t sort_bytes, uint32_t carry,
	uint32_t n, int first, int last, uint8_t* out, hipEvent_t* ev, hipStream_t stream);

// After the last slice: the two header bytes, the Adler-32 behind the last group, and the nine words of
// cfhip_deflate_result at `result` (bytes_in is passed).
extern "C" hipError_t cfhip_launch_deflate_final(const unsigned long long* state, unsigned long long bytes_in, uint8_t* out,
	unsigned long long* result, hipStream_t stream);

// The code builder alone on n <= 286 counts (device pointers), limit <= 15: one length per symbol.
extern "C" hipError_t cfhip_launch_deflate_code_lengths(const uint32_t* counts, uint32_t n, uint32_t limit,
	uint8_t* lengths, hipStream_t stream);

#endif
