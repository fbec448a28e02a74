"""The forms of the unit-weight BC7 selector search's keys (csrc/bc7_packed.h: the cross terms on the matrix pipe,
mfma_entry_base; the weight in a full byte, key_row_weights), on the CPU.  DESIGN.md section 4.1, tenth step.
The host program reaches key_row_weights through its host branch only; the device's v_perm_b32 selectors are covered by
tests/test_gpu_bc7_mfma_dots.py.

A stand-alone program (its own main, host compiler) includes bc7_packed.h and compares, per case:
  key       the key with the weight in a full byte, (cc_k << 8 | w_k) - 512 dt, minimised over the entries, with today's
            key_min_form (cc_k << 7 | w_k) - 256 dt: the same winning entry, the same error (key >> 8 against key >> 7) and
            the same weight (key & 255 against key & 127); an entry that does not exist holds CF_BC7_NO_ENTRY in both and
            never wins; mode 6's two halves meet by the smaller of their results, as assign_lsq_lane does it
  ranges    cc < 2^18, B < 2^26, 512 dt < 2^27, |key| < 2^26, a missing entry's key > 2^29: what bc7_packed.h states, checked
            in 64-bit arithmetic against the 32-bit results
  row       key_row_weights of four masked keys is the word of their low bytes, zero for a texel outside the subset, and
            equals the word today's form assembles from key & 127; the assignment's error, the sum of key >> 8, equals
            the sum of key >> 7
  mfma      per (texel, entry): the palette un-rotated to raw channel order (zeros where the fit codes no channel) dotted with
            the raw texel equals the slot-order palette dotted with texel<true>; interpolating the un-rotated endpoints gives
            the un-rotated palette; sum a b = sum a'b' + 128 sum a + 128 sum b' with a' = a ^ 0x80, b' = b ^ 0x80 as signed
            bytes; D = sum a'b' + 128 sum a has |D| < 2^19; base' = mfma_entry_base(B, sum b, fbits) has |base'| < 2^26 with the
            factor 256 and < 2^27 with 512; base' - F D equals B - F dt in 64-bit and in 32-bit arithmetic, so every entry's key,
            and with it the minimum and the winner, is today's.  Per index width 2, 3, 4: 2^20 seeded cases, 4096 of bytes 0 / 255
            and 4096 of bytes 127 / 128, spread over the rotations 0..3 and the channel sets 7, 8, 15
Cases of `key`: 2^20 seeded (texel, endpoint pair) cases per index width 2, 3, 4 (one in eight with endpoints equal in some
or all channels: ties); all 256 endpoint pairs of bytes 0 / 255 against the 16 texels of that kind; every byte of texel
and endpoints drawn from {127, 128} (65 536 cases per width are too many: 4096 seeded); every rotation 0..3 with channel
sets 7, 8 and 15 applied to texel and endpoints the way the kernel's selectors do (channels not coded zero on both
sides); all 28 weights occur (checked).  Cases of `row`: 2^20 seeded assignments of 16 texels with random subset masks
(empty and full ones included), one in sixteen with both endpoints equal so that every entry ties for every texel."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuttlefish_amd", "csrc")

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "bc7_packed.h"
static uint64_t st = 1234567891;
static uint32_t rnd() { st = st*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 32); }
static uint32_t dot4(uint32_t a, uint32_t b)
{
	uint32_t s = 0;
	for (int c = 0; c < 4; ++c) s += ((a >> (8*c)) & 255u)*((b >> (8*c)) & 255u);
	return s;
}
static unsigned long ncase = 0, nties = 0;
static uint32_t seen_w[3] = {0, 0, 0};   /* per index width: bit k set when entry k won */
static int fail(const char* what, long long a, long long b) { printf("%s: %lld %lld\n", what, a, b); return 1; }

/* one texel against the palette of (e0, e1) at index width ib: both key forms; *k7 and *k8 get the keys */
static int texel_case(uint32_t e0, uint32_t e1, uint32_t p, uint32_t ib, int* k7, int* k8)
{
	const int n = ib == 4u ? 16 : 8, have = 1 << ib;
	int r7[2], r8[2], a7[2], a8[2];
	const int m256 = -256, m512 = -512;
	for (int h = 0; h < n/8; ++h) {
		int b7 = 0x7FFFFFFF, b8 = 0x7FFFFFFF, i7 = -1, i8 = -1;
		for (int k = 8*h; k < 8*h + 8; ++k) {
			const bool valid = k < have;
			const uint32_t w = valid ? cf_bc7_weight(ib, (uint32_t)k) : 0u;
			const uint32_t c = pal_word(e0, e1, w);
			const uint32_t cc = dot4(c, c), dt = dot4(p, c);
			const long long B8 = ((long long)cc << 8) | w;
			if (cc >= (1u << 18) || B8 >= (1ll << 26) || 512ll*dt >= (1ll << 27)) return fail("range of cc, B, 512 dt", cc, dt);
			const int v7 = key_min_form((int)dt, m256, valid ? (int)((cc << 7) | w) : CF_BC7_NO_ENTRY);
			const int v8 = key_min_form((int)dt, m512, valid ? (int)B8 : CF_BC7_NO_ENTRY);
			const long long x8 = (valid ? B8 : (long long)CF_BC7_NO_ENTRY) - 512ll*dt;
			if (x8 != (long long)v8) return fail("the key leaves 32 bits", x8, v8);
			if (valid && (x8 >= (1ll << 26) || x8 <= -(1ll << 26))) return fail("range of a key", x8, 0);
			if (!valid && x8 <= (1ll << 29)) return fail("a missing entry's key", x8, 0);
			if (v7 < b7) { b7 = v7; i7 = k; }
			if (v8 < b8) { b8 = v8; i8 = k; }
		}
		r7[h] = b7; r8[h] = b8; a7[h] = i7; a8[h] = i8;
	}
	int b7 = r7[0], b8 = r8[0], i7 = a7[0], i8 = a8[0];
	if (n == 16) {
		if (r7[1] < b7) { b7 = r7[1]; i7 = a7[1]; }
		if (r8[1] < b8) { b8 = r8[1]; i8 = a8[1]; }
	}
	/* the plain search: smallest error, then smallest weight */
	long long be = 0; int bw = 0, bk = -1, equal = 0;
	for (int k = 0; k < have; ++k) {
		const uint32_t w = cf_bc7_weight(ib, (uint32_t)k), c = pal_word(e0, e1, w);
		const long long e = (long long)dot4(c, c) - 2ll*dot4(p, c);
		if (bk < 0 || e < be || (e == be && (int)w < bw)) { be = e; bw = (int)w; bk = k; }
	}
	for (int k = 0; k < have; ++k) {
		const uint32_t c = pal_word(e0, e1, cf_bc7_weight(ib, (uint32_t)k));
		equal += (long long)dot4(c, c) - 2ll*dot4(p, c) == be;
	}
	++ncase; nties += equal > 1;
	seen_w[ib - 2u] |= 1u << i8;
	if (i7 != i8 || (b7 >> 7) != (b8 >> 8) || (b7 & 127) != (b8 & 255) || (long long)(b8 >> 8) != be || (b8 & 255) != bw || i8 != bk) {
		printf("differs: 7-bit key %d entry %d, 8-bit key %d entry %d, plain error %lld weight %d entry %d\n", b7, i7, b8, i8, be, bw, bk);
		return 1;
	}
	*k7 = b7; *k8 = b8;
	return 0;
}
/* texel and endpoints as a fit of rotation rot and channel set chm sees them: colour rot - 1 and alpha change places,
   the slots that are not coded are zero on both sides */
static uint32_t slots(uint32_t v, uint32_t rot, uint32_t chm)
{
	uint32_t b[4] = {v & 255u, (v >> 8) & 255u, (v >> 16) & 255u, v >> 24};
	if (rot) { const uint32_t t = b[rot - 1u]; b[rot - 1u] = b[3]; b[3] = t; }
	uint32_t r = 0;
	for (int c = 0; c < 4; ++c) r |= ((chm >> c) & 1u ? b[c] : 0u) << (8*c);
	return r;
}
static uint32_t unrot(uint32_t v, uint32_t rot)
{
	uint32_t b[4] = {v & 255u, (v >> 8) & 255u, (v >> 16) & 255u, v >> 24};
	if (rot) { const uint32_t t = b[rot - 1u]; b[rot - 1u] = b[3]; b[3] = t; }
	return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
}
static int sb8(uint32_t w, int c) { return (int)(int8_t)(w >> (8*c)); }
static unsigned long nmfma = 0;
/* the cross terms as the matrix pipe forms them: raw texel praw, raw endpoints e0 / e1, a fit of rotation rot and channel set chm */
static int mfma_case(uint32_t e0, uint32_t e1, uint32_t praw, uint32_t rot, uint32_t chm, uint32_t ib)
{
	const uint32_t s0 = slots(e0, rot, chm), s1 = slots(e1, rot, chm), p = slots(praw, rot, chm);
	for (int k = 0; k < (1 << ib); ++k) {
		const uint32_t w = cf_bc7_weight(ib, (uint32_t)k);
		const uint32_t c = pal_word(s0, s1, w), craw = unrot(c, rot);
		if (pal_word(unrot(s0, rot), unrot(s1, rot), w) != craw || pal_at(pal_line(unrot(s0, rot), unrot(s1, rot)), w) != craw) return fail("un-rotated palette", c, craw);
		const long long dt = dot4(p, c);
		if ((long long)dot4(praw, craw) != dt) return fail("raw texel . un-rotated palette", dot4(praw, craw), dt);
		const uint32_t ax = praw ^ 0x80808080u, bx = craw ^ 0x80808080u;
		long long M = 0, sbp = 0;
		for (int ch = 0; ch < 4; ++ch) { M += sb8(ax, ch)*sb8(bx, ch); sbp += sb8(bx, ch); }
		const long long C = dot4(praw, 0x80808080u), sa = dot4(praw, 0x01010101u), sb = dot4(craw, 0x01010101u);
		if (C != 128*sa || sbp != sb - 512) return fail("C or sum b'", C, sbp);
		if (dt != M + 128*sa + 128*sbp) return fail("offset identity", dt, M + 128*sa + 128*sbp);
		const long long D = M + C;
		if (D >= (1ll << 19) || D <= -(1ll << 19)) return fail("range of D", D, 0);
		const long long cc = dot4(c, c);
		for (int fbits = 8; fbits <= 9; ++fbits) {
			const long long F = 1ll << fbits, B = (cc << (fbits - 1)) | w;
			const int bp = mfma_entry_base((int)B, (uint32_t)sb, fbits);
			if ((long long)bp != B - 128*F*(sb - 512)) return fail("base'", bp, B - 128*F*(sb - 512));
			const long long lim = fbits == 8 ? (1ll << 26) : (1ll << 27);
			if (bp >= lim || bp <= -lim) return fail("range of base'", bp, fbits);
			if (bp - F*D != B - F*dt) return fail("key, 64 bits", bp - F*D, B - F*dt);
			if (key_min_form((int)D, -(int)F, bp) != key_min_form((int)dt, -(int)F, (int)B)) return fail("key, 32 bits", D, dt);
			/* an entry that does not exist: its key stays inside 32 bits and above every real key */
			const long long none = (long long)CF_BC7_NO_ENTRY - F*D;
			if (none >= (1ll << 31) || none <= (1ll << 27) || (long long)key_min_form((int)D, -(int)F, CF_BC7_NO_ENTRY) != none) return fail("missing entry", none, D);
		}
	}
	++nmfma;
	return 0;
}
int main()
{
	int k7, k8;
	for (uint32_t ib = 2; ib <= 4; ++ib)
	for (int it = 0; it < (1 << 20) + 2*4096; ++it) {
		const uint32_t rot = (uint32_t)it & 3u, ci = ((uint32_t)it >> 2) % 3u;
		const uint32_t chm = ci == 0 ? 7u : (ci == 1 ? 8u : 15u);
		uint32_t v[3];
		for (int i = 0; i < 3; ++i) {
			const uint32_t r = rnd();
			v[i] = r;
			if (it >= (1 << 20) + 4096)      /* bytes 127 / 128 */
				v[i] = 0x7F7F7F7Fu + (r & 1u) + (((r >> 1) & 1u) << 8) + (((r >> 2) & 1u) << 16) + (((r >> 3) & 1u) << 24);
			else if (it >= (1 << 20))        /* bytes 0 / 255 */
				v[i] = ((r & 1u) ? 0xFFu : 0u) | ((r & 2u) ? 0xFF00u : 0u) | ((r & 4u) ? 0xFF0000u : 0u) | ((r & 8u) ? 0xFF000000u : 0u);
		}
		if (mfma_case(v[0], v[1], v[2], rot, chm, ib)) return 1;
	}
	for (uint32_t ib = 2; ib <= 4; ++ib) {
		for (int it = 0; it < (1 << 20); ++it) {
			uint32_t e0 = rnd(), e1 = rnd();
			const uint32_t p = rnd();
			if ((it & 7) == 0) {
				const uint32_t m = ((rnd() & 1u) ? 0xFFu : 0u) | ((rnd() & 1u) ? 0xFF00u : 0u) | ((rnd() & 1u) ? 0xFF0000u : 0u) | ((it & 8) ? 0xFF000000u : 0u);
				e1 = (e1 & ~m) | (e0 & m);
				if (it & 16) e1 = e0;
			}
			if (texel_case(e0, e1, p, ib, &k7, &k8)) return 1;
		}
		for (uint32_t pal = 0; pal < 256; ++pal)
			for (uint32_t t = 0; t < 16; ++t) {
				uint32_t e0 = 0, e1 = 0, p = 0;
				for (int c = 0; c < 4; ++c) {
					e0 |= ((pal >> c) & 1u ? 255u : 0u) << (8*c);
					e1 |= ((pal >> (4 + c)) & 1u ? 255u : 0u) << (8*c);
					p |= ((t >> c) & 1u ? 255u : 0u) << (8*c);
				}
				if (texel_case(e0, e1, p, ib, &k7, &k8)) return 1;
			}
		for (int it = 0; it < 4096; ++it) {        /* bytes 127 / 128 on both sides */
			uint32_t v[3];
			for (int i = 0; i < 3; ++i) {
				const uint32_t r = rnd();
				v[i] = 0x7F7F7F7Fu + (r & 1u) + (((r >> 1) & 1u) << 8) + (((r >> 2) & 1u) << 16) + (((r >> 3) & 1u) << 24);
			}
			if (texel_case(v[0], v[1], v[2], ib, &k7, &k8)) return 1;
		}
		for (uint32_t rot = 0; rot < 4; ++rot)
			for (uint32_t ci = 0; ci < 3; ++ci) {
				const uint32_t chm = ci == 0 ? 7u : (ci == 1 ? 8u : 15u);
				for (int it = 0; it < 4096; ++it)
					if (texel_case(slots(rnd(), rot, chm), slots(rnd(), rot, chm), slots(rnd(), rot, chm), ib, &k7, &k8)) return 1;
			}
	}
	if (seen_w[0] != 0xFu || seen_w[1] != 0xFFu || seen_w[2] != 0xFFFFu) return fail("entries that never won", seen_w[0], seen_w[2]);
	const unsigned long key_cases = ncase, key_ties = nties;
	/* whole assignments: the row's weights from the keys' low bytes, the error from key >> 8 */
	unsigned long nsum = 0, nallties = 0, nempty = 0, nfull = 0;
	for (int it = 0; it < (1 << 20); ++it) {
		const uint32_t ib = 2u + (uint32_t)(it % 3);
		uint32_t e0 = rnd(), e1 = rnd();
		const bool flat = (it & 15) == 0;
		if (flat) e1 = e0;
		uint32_t mask = rnd() & 0xFFFFu;
		if ((it & 255) == 1) mask = 0;
		if ((it & 255) == 2) mask = 0xFFFFu;
		nempty += mask == 0; nfull += mask == 0xFFFFu; nallties += flat;
		long long err7 = 0, err8 = 0;
		for (int r = 0; r < 4; ++r) {
			uint32_t key8[4], want = 0;
			for (int j = 0; j < 4; ++j) {
				if (texel_case(e0, e1, flat && (it & 16) ? e0 : rnd(), ib, &k7, &k8)) return 1;
				const bool in = (mask >> (4*r + j)) & 1u;
				const uint32_t m7 = in ? (uint32_t)k7 : 0u, m8 = in ? (uint32_t)k8 : 0u;
				err7 += (int)m7 >> 7; err8 += (int)m8 >> 8;
				if ((m7 & 127u) != (m8 & 255u) || (m8 & 255u) > 64u) return fail("weight of a key", m7, m8);
				key8[j] = m8;
				want |= (m8 & 255u) << (8*j);
			}
			if (key_row_weights(key8[0], key8[1], key8[2], key8[3]) != want) return fail("key_row_weights", want, r);
		}
		if (err7 != err8) return fail("the two widths' errors", err7, err8);
		++nsum;
	}
	printf("mfma cases %lu; ", nmfma);
	printf("equal on %lu key cases with %lu ties; %lu assignments, %lu flat, %lu empty, %lu full\n", key_cases, key_ties, nsum, nallties, nempty, nfull);
	return 0;
}
"""


def test_matrix_pipe_and_weight_byte_keys_equal_todays_keys(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    src = tmp_path / "mfma_identities.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mfma_identities"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    nmfma, cases, ties, nsum, flat, empty, full = (int(v) for v in re.findall(r"\d+", run.stdout)[:7])
    assert nmfma == 3*((1 << 20) + 2*4096), run.stdout
    assert cases == 3*((1 << 20) + 256*16 + 4096 + 12*4096), run.stdout
    assert ties > 100000 and nsum == 1 << 20 and flat == 1 << 16 and empty >= 4096 and full >= 4096, run.stdout


def test_no_switch_selects_another_form():
    """The product kernel builds the forms compared above and no other: the compile-time switches that once chose between
    them and their predecessors (the names below, behind the common prefix) occur nowhere in the encoder's source or in
    bc7_packed.h, so no -D can change what is built."""
    for name in ("bc7_encode.hip", "bc7_packed.h"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for switch in ("CANDW", "FITTRIMS", "KEYTRIMS", "MFMADOT"):
            assert "CF_BC7_" + switch not in text, (name, switch)
