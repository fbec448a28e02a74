// lzsize.h -- what the host side (cfhip_api.hip) and the kernels (lzsize.hip) of the deflate-size estimator share: the
// constants of the model, the layout of a slice's scratch and the launcher.
// The definition of the estimate is tests/lzsize_ref.py; every constant below has its twin
// there.
#ifndef CF_LZSIZE_H
#define CF_LZSIZE_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define CFLZ_MIN 4            // shortest match
#define CFLZ_MAX 258          // longest match
#define CFLZ_WINDOW 32768u    // W: a match reaches at most this far back
#define CFLZ_CANDS 4          // K: candidates per position, nearest first
#define CFLZ_CHUNK 4096u      // bytes parsed independently; one wavefront parses one chunk
#define CFLZ_COSTBLK 65536u   // bytes priced with one pair of code tables; one wavefront prices one block
#define CFLZ_LL 286           // literal / length alphabet
#define CFLZ_DD 30            // distance alphabet
// One cost block's counters (uint32): ll[286], dd[30], then the extra bits, literals, matches and matched bytes.
#define CFLZ_EXTRA 316
#define CFLZ_LITERALS 317
#define CFLZ_MATCHES 318
#define CFLZ_MATCHED 319
#define CFLZ_HIST 320
// The slice a stream is cut into unless cfhip_lz_slice_bytes says otherwise: whole cost blocks.
#define CFLZ_SLICE_DEFAULT (4u << 20)
// The five timed stages of a slice, in launch order.
#define CFLZ_STAGES 5

// The scratch of one slice of at most `slice` target bytes (a multiple of CFLZ_COSTBLK), which arrive behind the
// up to W bytes before them (sources only).  Offsets in bytes from a 256-byte aligned base; every array is 256-byte
// aligned.  m = slice + W positions: 1 (bytes) + 4 x 4 (keys and positions, in and out of the sort) per position,
// 4 (length and distance) per target byte, 1280 per cost block, the sort's own storage and 32 bytes of sums:
// 21.02 bytes per byte of slice + 17 W + the sort's storage (cflz_sort_bytes).
struct cflz_layout {
	size_t bytes, keys_in, keys_out, pos_in, pos_out, ld, hist, acc, sort, total;
};

inline cflz_layout cflz_scratch(size_t slice, size_t sort_bytes)
{
	const size_t m = slice + CFLZ_WINDOW;
	auto up = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
	cflz_layout l;
	size_t o = 0;
	l.bytes = o;    o = up(o + m + 16u);
	l.keys_in = o;  o = up(o + 4u*m);
	l.keys_out = o; o = up(o + 4u*m);
	l.pos_in = o;   o = up(o + 4u*m);
	l.pos_out = o;  o = up(o + 4u*m);
	l.ld = o;       o = up(o + 4u*slice);
	l.hist = o;     o = up(o + (slice/CFLZ_COSTBLK)*CFLZ_HIST*4u);
	l.acc = o;      o = up(o + 4u*sizeof(unsigned long long));
	l.sort = o;     o = up(o + sort_bytes);
	l.total = o;
	return l;
}

// A position's word after the match stage: L | (D - 1) << 16.  The parse flags it in bits 14 and 15.
#define CFLZ_TAKEN 0x8000u    // the position's match survives the lazy rule
#define CFLZ_SEEN 0x4000u     // the parse visits the position

#ifdef __HIPCC__
// deflate's length code - 257 and its extra bits for 3 <= len <= 258 (RFC 1951, 3.2.5)
__device__ __forceinline__ uint32_t lz_length_code(uint32_t len, uint32_t* extra)
{
	if (len == 258u) {
		*extra = 0u;
		return 28u;
	}
	const uint32_t l = len - 3u;
	if (l < 8u) {
		*extra = 0u;
		return l;
	}
	const uint32_t e = 29u - (uint32_t)__builtin_clz(l);     // floor(log2 l) - 2
	*extra = e;
	return 4u*e + 4u + ((l >> e) & 3u);
}

// deflate's distance code and its extra bits for d1 = distance - 1, 0 <= d1 < 32768
__device__ __forceinline__ uint32_t lz_dist_code(uint32_t d1, uint32_t* extra)
{
	if (d1 < 4u) {
		*extra = 0u;
		return d1;
	}
	const uint32_t e = 30u - (uint32_t)__builtin_clz(d1);    // floor(log2 d1) - 1
	*extra = e;
	return 2u*e + 2u + ((d1 >> e) & 1u);
}
#endif

// Bytes of temporary storage the radix sort needs for m pairs (a query, nothing runs).
extern "C" hipError_t cfhip_lz_sort_bytes(size_t m, size_t* bytes);

// One slice.  base: the scratch, laid out by cflz_scratch(slice_cap, sort_bytes).  Its byte array already holds
// `carry` source bytes (0 or W) followed by the n target bytes of the slice, n <= slice_cap.  The stages are
// enqueued on `stream` in order: keys, sort, match, parse + histogram, cost; the four sums (bits_q16, literals,
// matches, matched_bytes) are ADDED to acc (zeroed by the caller before the first slice).  ev: NULL, or
// 2 x CFLZ_STAGES events recorded around the stages.
extern "C" hipError_t cfhip_launch_lz_slice(uint8_t* base, const cflz_layout* lay, size_t sort_bytes, uint32_t carry,
	uint32_t n, hipEvent_t* ev, hipStream_t stream);

// The first three stages alone (keys, sort, match): the (L, D - 1) word of every target position in the layout's ld
// array.  ev: NULL, or the first 2 x 3 events of a stage list.  csrc/deflate.hip builds on it.
extern "C" hipError_t cfhip_launch_lz_matches(uint8_t* base, const cflz_layout* lay, size_t sort_bytes, uint32_t carry,
	uint32_t n, hipEvent_t* ev, hipStream_t stream);

// The same three stages on n bytes without a carry, cut into blocks of CFLZ_COSTBLK bytes that are matched as streams
// of their own: no match reaches in front of its position's block.  csrc/lz4.hip builds on it.
extern "C" hipError_t cfhip_launch_lz_block_matches(uint8_t* base, const cflz_layout* lay, size_t sort_bytes, uint32_t n,
	hipEvent_t* ev, hipStream_t stream);

// out[0..5] = bytes_in, bits_q16, est_bytes, literals, matches, matched_bytes from the four sums.
extern "C" hipError_t cfhip_launch_lz_final(const unsigned long long* acc, unsigned long long bytes_in,
	unsigned long long* out, hipStream_t stream);

#endif
