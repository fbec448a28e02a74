// inflate.h -- what the host side (cfhip_api.hip), the kernels (inflate.hip) and the stand-alone CPU program
// (tools/inflate_host.cpp) of the indexed inflater share: the constants, the decode logic of one chunk as inline
// functions that also compile with the host compiler alone, the layout of a slice's scratch and the launchers.
// THE DEFINITION is tests/inflate_ref.py: the rules of the format, the seven error classes
// and the order in which a chunk notices them are stated there; every function below has its twin there.
//
// The rules in short.  Wrapper: CMF & 15 == 8, FCHECK valid, no FDICT, the stream exactly its length (padding bits,
// Adler-32, nothing).  Dynamic header: HLIT <= 286, HDIST <= 30, no repeat code first, no run past HLIT + HDIST, symbol
// 256 has a code, no Kraft sum above 1; an incomplete code is accepted.  A bit pattern of no code, literal/length symbols
// 286 / 287 and distance codes 30 / 31 are code errors.  A distance before output byte 0 is a distance error.
#ifndef CF_INFLATE_H
#define CF_INFLATE_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CFINF_FN __host__ __device__ __forceinline__
#else
#define CFINF_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define CFINF_SYNC() __syncthreads()
#else
#define CFINF_SYNC() ((void)0)
#endif

#define CFINF_CHUNK 4096u          // output bytes per index entry and per wavefront (CFLZ_CHUNK)
// cfhip_inflate_status
#define CFINF_OK 0u
#define CFINF_E_WRAPPER 1u
#define CFINF_E_INDEX 2u
#define CFINF_E_HEADER 3u
#define CFINF_E_CODE 4u
#define CFINF_E_DISTANCE 5u
#define CFINF_E_OVERRUN 6u
#define CFINF_E_CHECKSUM 7u
// One word per output byte: the byte, or CFINF_PTR | the output position whose byte it is (strictly below its own).
#define CFINF_PTR 0x80000000u
// The chunk's token words in LDS, at the token's first position: a literal's byte, or CFINF_MATCH | length - 3 |
// (distance - 1) << 8.  Padded by one word per 64: a lane expands 64 consecutive positions, each lane in another bank.
#define CFINF_MATCH 0x40000000u
#define CFINF_PAD(i) ((i) + ((i) >> 6))
// The four timed stages of a slice, in launch order: decode, resolve (all its rounds), pack (with the chunks' Adler
// sums), fold.
#define CFINF_STAGES 4
// The state carried from slice to slice (uint64).
#define CFINF_S_FAIL 0             // min over the failing chunks of chunk << 3 | class; ~0 while none failed
#define CFINF_S_A 1                // Adler-32 sums of the bytes so far, as deflate.h's
#define CFINF_S_B 2
#define CFINF_S_LEN 3
#define CFINF_S_LITERALS 4
#define CFINF_S_MATCHES 5
#define CFINF_S_MATCHED 6
#define CFINF_S_ROUNDS 7           // most resolve rounds that did work in one slice
#define CFINF_S_LEFT 8             // [CFINF_MAX_ROUNDS + 1]: words still unresolved after round r of the current slice
#define CFINF_MAX_ROUNDS 32
#define CFINF_S_WORDS 48

struct cfinf_entry {               // cfhip_zindex_entry
	uint64_t header_bit, token_bit;
};

// ---- the decode logic ---------------------------------------------------------------------------------------------
// A canonical code: per length the count, the first code and where its symbols start in `sorted`; a table of the
// first LB bits (symbol << 4 | length, 0: longer than LB bits or no code).
template <int NSYM, int LB>
struct CfinfCode {
	uint16_t cnt[16], first[16], offs[16];
	uint16_t sorted[NSYM];
	uint16_t lut[(1 << LB) + 1];
};

// Everything one chunk's decode keeps: LDS on the device (one wavefront), an ordinary object on the host.
struct CfinfWork {
	CfinfCode<288, 10> ll;
	CfinfCode<32, 8> dd;
	CfinfCode<19, 7> cl;
	uint8_t lens[320];             // literal/length lengths from 0, distance lengths from 288
	uint8_t cllen[20];
	uint32_t S[CFINF_CHUNK + CFINF_CHUNK/64u];
	uint16_t cover[64];            // the first position of the token that covers position 64 k
	// the walk's state between its serial and its parallel parts
	uint64_t pos, hdr, run_src;
	uint32_t final_, btype, left, data_lo, len, produced, phase, event, err, run_p, run_k, nll, ndd;
	uint32_t literals, matches, matched;
};

enum { CFINF_PH_LINK = 0, CFINF_PH_ENTER, CFINF_PH_PRODUCE, CFINF_PH_TRAIL };
enum { CFINF_EV_HEADER = 0, CFINF_EV_RUN, CFINF_EV_DONE, CFINF_EV_ERR };

// The bits of the stream: 32 bits from any position, zeros behind the stream.  Every byte read is range-checked; the
// words come through a 64-bit window with the word behind it already on its way.
struct CfinfBits {
	const uint8_t* z;
	uint64_t zbytes, T, wbase, win;
	uint32_t nxt;
};

CFINF_FN uint32_t cfinf_word(const CfinfBits& b, uint64_t w)
{
	const uint64_t at = 4u*w;
	if (at + 4u <= b.zbytes && (((uintptr_t)b.z) & 3u) == 0u)
		return *reinterpret_cast<const uint32_t*>(b.z + at);
	uint32_t v = 0u;
	for (uint32_t k = 0u; k < 4u; ++k)
		if (at + k < b.zbytes)
			v |= (uint32_t)b.z[at + k] << (8u*k);
	return v;
}

CFINF_FN void cfinf_bits_init(CfinfBits& b, const uint8_t* z, uint64_t zbytes)
{
	b.z = z;
	b.zbytes = zbytes;
	b.T = 8u*zbytes;
	b.wbase = ~(uint64_t)0 << 8;   // far from any position: the first peek loads
	b.win = 0u;
	b.nxt = 0u;
}

CFINF_FN uint32_t cfinf_peek(CfinfBits& b, uint64_t pos)
{
	const uint64_t d = pos - b.wbase;
	if (d >= 32u) {
		if (d < 64u) {
			b.wbase += 32u;
			b.win = (b.win >> 32) | ((uint64_t)b.nxt << 32);
		} else {
			b.wbase = pos & ~(uint64_t)31u;
			b.win = cfinf_word(b, b.wbase >> 5) | ((uint64_t)cfinf_word(b, (b.wbase >> 5) + 1u) << 32);
		}
		b.nxt = cfinf_word(b, (b.wbase >> 5) + 2u);
	}
	return (uint32_t)(b.win >> (pos - b.wbase));
}

// k <= 16 bits at *pos; CFINF_E_OVERRUN where they end behind the stream
CFINF_FN uint32_t cfinf_get(CfinfBits& b, uint64_t* pos, uint32_t k, uint32_t* v)
{
	if (*pos + k > b.T)
		return CFINF_E_OVERRUN;
	*v = cfinf_peek(b, *pos) & ((1u << k) - 1u);
	*pos += k;
	return CFINF_OK;
}

CFINF_FN uint32_t cfinf_rev15(uint32_t v)
{
	uint32_t r = 0u;
	for (uint32_t i = 0u; i < 15u; ++i)
		r |= ((v >> i) & 1u) << (14u - i);
	return r;
}

// The symbol whose code starts at pos, and its length; nothing is consumed.
template <int NSYM, int LB>
CFINF_FN uint32_t cfinf_symbol(const CfinfCode<NSYM, LB>& c, CfinfBits& b, uint64_t pos, uint32_t* sym, uint32_t* len)
{
	const uint32_t bits = cfinf_peek(b, pos) & 0x7FFFu;
	uint32_t hit = LB ? c.lut[bits & ((1u << LB) - 1u)] : 0u;
	if (!hit) {
#if defined(__HIP_DEVICE_COMPILE__)
		const uint32_t rev = __brev(bits) >> 17;
#else
		const uint32_t rev = cfinf_rev15(bits);
#endif
		for (uint32_t l = 1u; l < 16u; ++l) {
			const uint32_t code = rev >> (15u - l), first = c.first[l];
			if (code >= first && code - first < c.cnt[l]) {
				hit = ((uint32_t)c.sorted[c.offs[l] + code - first] << 4) | l;
				break;
			}
		}
		if (!hit)
			return b.T - pos < 15u ? CFINF_E_OVERRUN : CFINF_E_CODE;
	}
	*sym = hit >> 4;
	*len = hit & 15u;
	return pos + *len > b.T ? CFINF_E_OVERRUN : CFINF_OK;
}

// deflate's length code lc = symbol - 257 <= 28 and distance code dc <= 29: base and extra bits (RFC 1951, 3.2.5)
CFINF_FN uint32_t cfinf_length_base(uint32_t lc, uint32_t* extra)
{
	if (lc < 8u) { *extra = 0u; return 3u + lc; }
	if (lc == 28u) { *extra = 0u; return 258u; }
	const uint32_t e = (lc - 4u) >> 2;
	*extra = e;
	return 3u + ((4u + (lc & 3u)) << e);
}

CFINF_FN uint32_t cfinf_dist_base(uint32_t dc, uint32_t* extra)
{
	if (dc < 4u) { *extra = 0u; return 1u + dc; }
	const uint32_t e = (dc - 2u) >> 1;
	*extra = e;
	return 1u + ((2u + (dc & 1u)) << e);
}

// RFC 1951's order of the code-length code lengths, five bits each
CFINF_FN uint32_t cfinf_cl_order(uint32_t i)
{
	// 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
	const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
		10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
	const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
	return (uint32_t)((i < 12u ? lo >> (5u*i) : hi >> (5u*(i - 12u))) & 31u);
}

// 16 counters of 16 bits in four words (an alphabet has at most 320 symbols): registers, where an array indexed by a
// code length would be memory
struct CfinfCount16 {
	uint64_t k[4];
};

CFINF_FN uint32_t cfinf_count_get(const CfinfCount16& c, uint32_t l)
{
	const uint64_t v = (l >> 2) == 0u ? c.k[0] : (l >> 2) == 1u ? c.k[1] : (l >> 2) == 2u ? c.k[2] : c.k[3];
	return (uint32_t)(v >> (16u*(l & 3u))) & 0xFFFFu;
}

CFINF_FN void cfinf_count_add(CfinfCount16& c, uint32_t l, uint32_t d)
{
	const uint64_t inc = (uint64_t)d << (16u*(l & 3u));
	c.k[0] += (l >> 2) == 0u ? inc : 0u;
	c.k[1] += (l >> 2) == 1u ? inc : 0u;
	c.k[2] += (l >> 2) == 2u ? inc : 0u;
	c.k[3] += (l >> 2) == 3u ? inc : 0u;
}

// The serial half of a code: counts, the Kraft sum, first codes, offsets and the symbols in (length, symbol) order.
// false: the Kraft sum is above 1.
template <int NSYM, int LB>
CFINF_FN bool cfinf_code_serial(CfinfCode<NSYM, LB>& c, const uint8_t* lens, uint32_t n)
{
	CfinfCount16 cnt = {{0u, 0u, 0u, 0u}}, next = {{0u, 0u, 0u, 0u}};
	for (uint32_t i = 0u; i < n; ++i)
		cfinf_count_add(cnt, lens[i], 1u);
	uint32_t kraft = 0u, code = 0u, at = 0u;
	c.cnt[0] = c.first[0] = c.offs[0] = 0u;
	for (uint32_t l = 1u; l < 16u; ++l) {
		const uint32_t k = cfinf_count_get(cnt, l);
		kraft += k << (15u - l);
		c.cnt[l] = (uint16_t)k;
		c.first[l] = (uint16_t)code;
		c.offs[l] = (uint16_t)at;
		cfinf_count_add(next, l, at);
		code = (code + k) << 1;
		at += k;
	}
	if (kraft > (1u << 15))
		return false;
	for (uint32_t i = 0u; i < n; ++i) {
		const uint32_t l = lens[i];
		if (l) {
			c.sorted[cfinf_count_get(next, l)] = (uint16_t)i;
			cfinf_count_add(next, l, 1u);
		}
	}
	return true;
}

// The parallel half: the table of the first LB bits, by lanes `lane` of `nl`.
template <int NSYM, int LB>
CFINF_FN void cfinf_code_lut_zero(CfinfCode<NSYM, LB>& c, uint32_t lane, uint32_t nl)
{
	for (uint32_t i = lane; i < (1u << LB); i += nl)
		c.lut[i] = 0u;
}

template <int NSYM, int LB>
CFINF_FN void cfinf_code_lut_fill(CfinfCode<NSYM, LB>& c, const uint8_t* lens, uint32_t lane, uint32_t nl)
{
	uint32_t used = 0u;
	for (uint32_t l = 1u; l < 16u; ++l)
		used += c.cnt[l];
	for (uint32_t j = lane; j < used; j += nl) {
		const uint32_t sym = c.sorted[j], l = lens[sym];
		if (l > (uint32_t)LB)
			continue;
		const uint32_t code = c.first[l] + (j - c.offs[l]);
		uint32_t rev = 0u;
		for (uint32_t i = 0u; i < l; ++i)
			rev |= ((code >> i) & 1u) << (l - 1u - i);
		for (uint32_t v = rev; v < (1u << LB); v += 1u << l)
			c.lut[v] = (uint16_t)((sym << 4) | l);
	}
}

// both, with the barriers between and behind them: all lanes call it
template <int NSYM, int LB>
CFINF_FN void cfinf_code_lut(CfinfCode<NSYM, LB>& c, const uint8_t* lens, uint32_t lane, uint32_t nl)
{
	cfinf_code_lut_zero(c, lane, nl);
	CFINF_SYNC();
	cfinf_code_lut_fill(c, lens, lane, nl);
	CFINF_SYNC();
}

// The serial half of the block header at w.pos (one lane): the type, a stored block's length, a dynamic block's code
// lengths in w.lens and the serial halves of its codes.  Afterwards w.pos is the block's first token (stored: its first
// data byte).  Sets w.err.
CFINF_FN void cfinf_header_serial(CfinfWork& w, CfinfBits& b)
{
	uint64_t pos = w.pos;
	uint32_t v = 0u, e;
	w.hdr = pos;
	if ((e = cfinf_get(b, &pos, 3u, &v)) != CFINF_OK) { w.err = e; return; }
	w.final_ = v & 1u;
	w.btype = v >> 1;
	if (w.btype == 3u) { w.err = CFINF_E_HEADER; return; }
	if (w.btype == 0u) {
		const uint64_t p = (pos + 7u) >> 3;
		if (p + 4u > b.zbytes) { w.err = CFINF_E_OVERRUN; return; }
		const uint32_t ln = (uint32_t)b.z[p] | (uint32_t)b.z[p + 1u] << 8, nl = (uint32_t)b.z[p + 2u] | (uint32_t)b.z[p + 3u] << 8;
		if (ln != (nl ^ 0xFFFFu)) { w.err = CFINF_E_HEADER; return; }
		if (p + 4u + ln > b.zbytes) { w.err = CFINF_E_OVERRUN; return; }
		w.len = w.left = ln;
		w.pos = 8u*(p + 4u);
		return;
	}
	if (w.btype == 1u) {
		w.nll = 288u;
		w.ndd = 32u;
		for (uint32_t i = 0u; i < 288u; ++i)
			w.lens[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : 8u);
		for (uint32_t i = 0u; i < 32u; ++i)
			w.lens[288u + i] = 5u;
	} else {
		uint32_t hlit = 0u, hdist = 0u, hclen = 0u;
		if ((e = cfinf_get(b, &pos, 5u, &hlit)) != CFINF_OK || (e = cfinf_get(b, &pos, 5u, &hdist)) != CFINF_OK ||
			(e = cfinf_get(b, &pos, 4u, &hclen)) != CFINF_OK) { w.err = e; return; }
		hlit += 257u;
		hdist += 1u;
		hclen += 4u;
		if (hlit > 286u || hdist > 30u) { w.err = CFINF_E_HEADER; return; }
		uint8_t* cl = w.cllen;
		for (uint32_t i = 0u; i < 19u; ++i)
			cl[i] = 0u;
		for (uint32_t i = 0u; i < hclen; ++i) {
			if ((e = cfinf_get(b, &pos, 3u, &v)) != CFINF_OK) { w.err = e; return; }
			cl[cfinf_cl_order(i)] = (uint8_t)v;
		}
		if (!cfinf_code_serial(w.cl, cl, 19u)) { w.err = CFINF_E_HEADER; return; }
		cfinf_code_lut_zero(w.cl, 0u, 1u);             // this lane alone: 128 entries
		cfinf_code_lut_fill(w.cl, cl, 0u, 1u);
		const uint32_t total = hlit + hdist;
		uint32_t i = 0u, prev = 0u;
		while (i < total) {
			uint32_t s = 0u, l = 0u;
			if ((e = cfinf_symbol(w.cl, b, pos, &s, &l)) != CFINF_OK) { w.err = e; return; }
			pos += l;
			if (s < 16u) {
				w.lens[i < hlit ? i : 288u + (i - hlit)] = (uint8_t)s;
				prev = s;
				++i;
				continue;
			}
			uint32_t val = 0u, run = 0u;
			if (s == 16u) {
				if (i == 0u) { w.err = CFINF_E_HEADER; return; }
				val = prev;
				if ((e = cfinf_get(b, &pos, 2u, &run)) != CFINF_OK) { w.err = e; return; }
				run += 3u;
			} else if (s == 17u) {
				if ((e = cfinf_get(b, &pos, 3u, &run)) != CFINF_OK) { w.err = e; return; }
				run += 3u;
			} else {
				if ((e = cfinf_get(b, &pos, 7u, &run)) != CFINF_OK) { w.err = e; return; }
				run += 11u;
			}
			if (i + run > total) { w.err = CFINF_E_HEADER; return; }
			for (; run; --run, ++i)
				w.lens[i < hlit ? i : 288u + (i - hlit)] = (uint8_t)val;
			prev = val;
		}
		if (!w.lens[256]) { w.err = CFINF_E_HEADER; return; }
		w.nll = hlit;
		w.ndd = hdist;
	}
	if (!cfinf_code_serial(w.ll, w.lens, w.nll) || !cfinf_code_serial(w.dd, w.lens + 288, w.ndd)) {
		w.err = CFINF_E_HEADER;
		return;
	}
	w.pos = pos;
}

// a token's first position p, its `len` positions: the 64-position boundaries it covers
CFINF_FN void cfinf_cover(CfinfWork& w, uint32_t p, uint32_t len)
{
	for (uint32_t k = (p + 63u) >> 6; k <= (p + len - 1u) >> 6; ++k)
		w.cover[k] = (uint16_t)p;
}

// The serial walk (one lane) from w.pos inside a block, through the phases of tests/inflate_ref.py, until it needs
// all lanes again: a new header, a stored run to copy, the chunk's end or an error.  Every step consumes bits of the
// stream or produces bytes of the chunk, so any garbage terminates.  base: the chunk's first output position.
CFINF_FN void cfinf_walk(CfinfWork& w, CfinfBits& b, const cfinf_entry* index, uint64_t C, uint64_t c, uint32_t want,
	uint64_t base)
{
	uint64_t pos = w.pos;
	uint32_t produced = w.produced, phase = w.phase, left = w.left;
	const uint32_t btype = w.btype, final_ = w.final_;           // the walk stays inside one block
	const uint64_t hdr = w.hdr;
	uint32_t literals = 0u, matches = 0u, matched = 0u;
	uint32_t event = CFINF_EV_ERR, err = CFINF_OK;
	for (;;) {
		bool block_end = false;
		if (phase == CFINF_PH_PRODUCE) {
			if (btype == 0u) {
				if (left) {
					const uint32_t k = left < want - produced ? left : want - produced;
					w.run_p = produced;
					w.run_k = k;
					w.run_src = pos >> 3;
					pos += 8u*(uint64_t)k;
					left -= k;
					produced += k;
					literals += k;
					if (produced == want)
						phase = CFINF_PH_TRAIL;
					event = CFINF_EV_RUN;
					break;
				}
				block_end = true;
			} else {
				uint32_t s = 0u, l = 0u;
				if ((err = cfinf_symbol(w.ll, b, pos, &s, &l)) != CFINF_OK)
					break;
				pos += l;
				if (s < 256u) {
					w.S[CFINF_PAD(produced)] = s;
					if (!(produced & 63u))
						w.cover[produced >> 6] = (uint16_t)produced;
					++produced;
					++literals;
				} else if (s == 256u)
					block_end = true;
				else {
					if (s >= 286u) { err = CFINF_E_CODE; break; }
					uint32_t eb, ev = 0u, ds = 0u;
					uint32_t len = cfinf_length_base(s - 257u, &eb);
					if ((err = cfinf_get(b, &pos, eb, &ev)) != CFINF_OK)
						break;
					len += ev;
					if ((err = cfinf_symbol(w.dd, b, pos, &ds, &l)) != CFINF_OK)
						break;
					pos += l;
					if (ds >= 30u) { err = CFINF_E_CODE; break; }
					uint32_t dist = cfinf_dist_base(ds, &eb);
					if ((err = cfinf_get(b, &pos, eb, &ev)) != CFINF_OK)
						break;
					dist += ev;
					if ((uint64_t)dist > base + produced) { err = CFINF_E_DISTANCE; break; }
					if (produced + len > want) { err = CFINF_E_INDEX; break; }
					w.S[CFINF_PAD(produced)] = CFINF_MATCH | (len - 3u) | ((dist - 1u) << 8);
					cfinf_cover(w, produced, len);
					produced += len;
					++matches;
					matched += len;
				}
				if (!block_end && produced == want)
					phase = CFINF_PH_TRAIL;
			}
		} else {
			// LINK and TRAIL: through everything that produces no output
			bool stop = false;
			if (btype == 0u) {
				if (left) stop = true; else block_end = true;
			} else {
				uint32_t s = 0u, l = 0u;
				if ((err = cfinf_symbol(w.ll, b, pos, &s, &l)) != CFINF_OK)
					break;
				if (s == 256u) {
					pos += l;
					block_end = true;
				} else
					stop = true;
			}
			if (stop) {
				const uint64_t k = phase == CFINF_PH_LINK ? 0u : c + 1u;
				if (k >= C || index[k].header_bit != hdr || index[k].token_bit != pos) { err = CFINF_E_INDEX; break; }
				if (phase == CFINF_PH_TRAIL) { event = CFINF_EV_DONE; break; }
				phase = CFINF_PH_PRODUCE;
				continue;
			}
		}
		if (block_end) {
			if (!final_) { event = CFINF_EV_HEADER; break; }
			if (phase != CFINF_PH_TRAIL || c + 1u < C) { err = CFINF_E_OVERRUN; break; }
			if (((pos + 7u) >> 3) + 4u != b.zbytes) { err = CFINF_E_WRAPPER; break; }
			event = CFINF_EV_DONE;
			break;
		}
	}
	w.pos = pos;
	w.produced = produced;
	w.phase = phase;
	w.left = left;
	w.literals += literals;
	w.matches += matches;
	w.matched += matched;
	w.err = err;
	w.event = err != CFINF_OK ? (uint32_t)CFINF_EV_ERR : event;
}

// Chunk c of C (C == 0: the walk of an empty stream, c = 0, want = 0) by lanes `lane` of `nl`, all of which call it:
// -> the error class, the same in every lane.  On CFINF_OK w.S and w.cover hold the chunk's tokens, w.literals,
// w.matches and w.matched their counts.
CFINF_FN uint32_t cfinf_chunk(CfinfWork& w, const uint8_t* z, uint64_t zbytes, const cfinf_entry* index, uint64_t C,
	uint64_t c, uint32_t want, uint32_t lane, uint32_t nl)
{
	CfinfBits b;
	cfinf_bits_init(b, z, zbytes);
	const uint64_t base = c*(uint64_t)CFINF_CHUNK;
	if (lane == 0u) {
		w.err = CFINF_OK;
		w.event = CFINF_EV_HEADER;
		w.produced = 0u;
		w.literals = w.matches = w.matched = 0u;
		w.left = w.len = w.btype = w.final_ = 0u;
		if (c == 0u) {
			if (zbytes < 6u || (z[0] & 15u) != 8u || (((uint32_t)z[0] << 8) | z[1]) % 31u != 0u || (z[1] & 0x20u))
				w.err = CFINF_E_WRAPPER;
			w.phase = want ? CFINF_PH_LINK : CFINF_PH_TRAIL;
			w.pos = 16u;
		} else {
			const uint64_t hb = index[c].header_bit, tb = index[c].token_bit;
			if (!(hb >= 16u && hb < tb && tb <= b.T))
				w.err = CFINF_E_INDEX;
			w.phase = CFINF_PH_ENTER;
			w.pos = hb;
		}
		if (w.err != CFINF_OK)
			w.event = CFINF_EV_ERR;
	}
	CFINF_SYNC();
	for (;;) {
		const uint32_t ev = w.event;
		if (ev == CFINF_EV_DONE || ev == CFINF_EV_ERR)
			break;
		if (ev == CFINF_EV_HEADER) {
			if (lane == 0u)
				cfinf_header_serial(w, b);
			CFINF_SYNC();
			if (w.err == CFINF_OK && w.btype != 0u) {
				cfinf_code_lut(w.ll, w.lens, lane, nl);
				cfinf_code_lut(w.dd, w.lens + 288, lane, nl);
			}
			if (lane == 0u && w.err == CFINF_OK && w.phase == CFINF_PH_ENTER) {
				const uint64_t tb = index[c].token_bit;
				if (w.btype == 0u) {
					const uint64_t data = w.pos >> 3;
					if ((tb & 7u) || (tb >> 3) < data || (tb >> 3) >= data + w.len)
						w.err = CFINF_E_INDEX;
					else
						w.left = w.len - (uint32_t)((tb >> 3) - data);
				} else if (tb < w.pos)
					w.err = CFINF_E_INDEX;
				w.pos = tb;
				w.phase = CFINF_PH_PRODUCE;
			}
		} else {
			// a stored run: run_k bytes from byte run_src of the stream (inside it: the header checked the block)
			for (uint32_t j = lane; j < w.run_k; j += nl) {
				const uint32_t p = w.run_p + j;
				w.S[CFINF_PAD(p)] = z[w.run_src + j];
				if (!(p & 63u))
					w.cover[p >> 6] = (uint16_t)p;
			}
		}
		CFINF_SYNC();
		if (lane == 0u) {
			if (w.err == CFINF_OK)
				cfinf_walk(w, b, index, C, c, want, base);
			else
				w.event = CFINF_EV_ERR;
		}
		CFINF_SYNC();
	}
	return w.err;
}

// Position i of the chunk at `base`, inside the token with word t at first position p0: the byte or the pointer.
CFINF_FN uint32_t cfinf_expand(uint32_t t, uint32_t p0, uint32_t i, uint64_t base)
{
	(void)p0;
	if (!(t & CFINF_MATCH))
		return t & 0xFFu;
	return CFINF_PTR | (uint32_t)(base + i - (((t >> 8) & 0x7FFFu) + 1u));
}

// ---- the scratch of one slice and the launchers (the GPU build only) ------------------------------------------------
#if defined(__HIPCC__)
// Per output byte of a slice two words (the resolve rounds go from one array to the other): 8 bytes per byte, and per
// chunk two Adler sums; the state.
struct cfinf_layout {
	size_t s0, s1, adler, state, total;
};

inline cfinf_layout cfinf_scratch(size_t slice)
{
	auto up = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
	cfinf_layout l;
	size_t o = 0;
	l.s0 = o;    o = up(o + 4u*slice);
	l.s1 = o;    o = up(o + 4u*slice);
	l.adler = o; o = up(o + (slice/CFINF_CHUNK)*8u);
	l.state = o; o = up(o + CFINF_S_WORDS*8u);
	l.total = o;
	return l;
}

inline uint32_t cfinf_rounds_bound(size_t n)
{
	uint32_t r = 1u;
	while (((size_t)1 << (r - 1u)) < n)
		++r;
	return r;                      // ceil(log2 n) + 1
}

// One slice: output bytes [at, at + n) of out_bytes, at a multiple of CFINF_CHUNK.  base: the scratch.  first: the
// call's first slice (the state starts there).  ev: NULL or 2 x CFINF_STAGES.
extern "C" hipError_t cfhip_launch_inflate_slice(uint8_t* base, const cfinf_layout* lay, const uint8_t* z, size_t zbytes,
	const cfinf_entry* index, size_t out_bytes, size_t at, uint32_t n, int first, uint8_t* out, hipEvent_t* ev,
	hipStream_t stream);

// After the last slice: the Adler-32 against the trailer's and the words of cfhip_inflate_result.
extern "C" hipError_t cfhip_launch_inflate_final(const unsigned long long* state, const uint8_t* z, size_t zbytes,
	size_t out_bytes, unsigned long long* result, hipStream_t stream);

// The index of a slice the encoder has just written (deflate.h's group records blk of its n bytes): entries chunk0 on.
extern "C" hipError_t cfhip_launch_zindex(const uint32_t* blk, uint32_t n, size_t chunk0, cfinf_entry* index,
	hipStream_t stream);
#endif

#endif
