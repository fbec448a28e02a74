"""The whole-word `quantize` and `refit_window` of csrc/bc7_encode.hip against their per-channel forms, on the CPU.

A stand-alone program (its own main, host compiler, -ffp-contract=off like the kernels) holds
  ref::  the per-channel forms restated here: integer clamp, a shift and an OR per field, one `dequant` per byte, the
         window's candidates q - 1, q, q + 1 per channel with validity from the wrapped value;
  dev::  the two functions cut out of bc7_encode.hip as they stand (between their opening lines and the comments that
         follow them), with csrc/bc7_packed.h, the device qualifiers defined away and the two builtins they use written
         out (v_med3_f32: the median; v_cvt_pk_u8_f32: convert, saturate, insert as byte c).
Both run on 1 000 000 seeded fits: every mode's (colour bits, alpha bits, p-bit kind) and the scalar planes of modes 4 / 5,
both metrics, endpoints from four distributions (beyond the byte range, next to 0 / 255, integers, inside the range), the
window's sums A, B, C from real selector sets.  q0, q1, e0, e1 and the p-bits must be equal after `quantize` and again after
`refit_window`.  Systems with n C - S^2 <= 0 are left out of the window's comparison: there A or C is 0, the sentinel's form
value is not +inf, both forms return garbage (different garbage) and the kernel discards it (`live` in fit_lane).  The test
also asserts that the window moved a field and that fields at 0 or qmax (the out-of-range candidates) occurred."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuttlefish_amd", "csrc")

PRELUDE = r"""
#include <stdint.h>
#include <stdio.h>
#include <math.h>
#include <string.h>
#include "bc7_packed.h"
struct SubFit { uint32_t e0, e1, q0, q1, pb, err; };
static inline float fb(uint32_t v, int c) { return (float)((v >> (8*c)) & 255u); }
static inline float sc_of(uint32_t t)
{
	return t == 4u ? 15.0f/255.0f : t == 5u ? 31.0f/255.0f : t == 6u ? 63.0f/255.0f : t == 7u ? 127.0f/255.0f : t == 8u ? 255.0f/255.0f : 0.0f;
}
"""

REFERENCE = r"""
namespace ref {
static inline uint32_t dequant(uint32_t v, uint32_t t) { return ((v << (8u - t)) | (v >> (2u*t - 8u))) & 255u; }
template <bool UNITW>
static inline void quantize(const float (&x0)[4], const float (&x1)[4], uint32_t cb,
	uint32_t ab, uint32_t pbk, const uint32_t (&wt)[4], SubFit& f)
{
	const uint32_t S = pbk ? 1u : 0u;
	const float H = pbk ? 0.5f : 1.0f;
	const uint32_t Tc = cb + S, Ta = ab + S;
	const float scc = cb ? sc_of(Tc) : 0.0f, sca = ab ? sc_of(Ta) : 0.0f;
	const int qmc = (1 << cb) - 1, qma = (1 << ab) - 1;
	const uint32_t shc = cb ? Tc : 8u, sha = ab ? Ta : 8u;
	const uint32_t cmask = cb ? 255u : 0u, amask = ab ? 255u : 0u;
	// [endpoint][p]
	uint32_t q[2][2] = {{0, 0}, {0, 0}}, d[2][2] = {{0, 0}, {0, 0}};
	float er[2][2];
	for (int e = 0; e < 2; ++e) {
		for (int p = 0; p < 2; ++p) {
			const uint32_t P = pbk ? (uint32_t)p : 0u;
			const float Pf = (float)P;
			float acc = 0.0f;
			for (int c = 0; c < 4; ++c) {
				const uint32_t t = c < 3 ? shc : sha;
				const float sc = c < 3 ? scc : sca;
				const int qmax = c < 3 ? qmc : qma;
				const float xv = e ? x1[c] : x0[c];
				const float y = xv*sc;
				const float u = (y - Pf)*H;
				int qq = (int)floorf(u + 0.5f);
				qq = qq < 0 ? 0 : (qq > qmax ? qmax : qq);
				const uint32_t dd = dequant(((uint32_t)qq << S) | P, t) & (c < 3 ? cmask : amask);
				const float dx = (float)dd - xv;
				const float t2 = dx*dx;
				acc = UNITW ? acc + t2 : fmaf((float)wt[c], t2, acc);
				q[e][p] |= (uint32_t)qq << (8*c);
				d[e][p] |= dd << (8*c);
			}
			er[e][p] = acc;
		}
	}
	uint32_t p0, p1;
	{
		const uint32_t i0 = er[0][1] < er[0][0] ? 1u : 0u;
		const uint32_t i1 = er[1][1] < er[1][0] ? 1u : 0u;
		const float s0 = er[0][0] + er[1][0];
		const float s1 = er[0][1] + er[1][1];
		const uint32_t sh = s1 < s0 ? 1u : 0u;
		p0 = pbk == 1u ? i0 : (pbk == 2u ? sh : 0u);
		p1 = pbk == 1u ? i1 : (pbk == 2u ? sh : 0u);
	}
	f.q0 = p0 ? q[0][1] : q[0][0];
	f.e0 = p0 ? d[0][1] : d[0][0];
	f.q1 = p1 ? q[1][1] : q[1][0];
	f.e1 = p1 ? d[1][1] : d[1][0];
	f.pb = p0 | (p1 << 1);
}


static inline void refit_window(const float (&xu0)[4], const float (&xu1)[4], const float (&hq)[3],
	uint32_t cb, uint32_t ab, uint32_t pbk, SubFit& f)
{
	const uint32_t S = pbk ? 1u : 0u;
	const uint32_t P0 = f.pb & 1u, P1 = (f.pb >> 1) & 1u;
	const float fA = hq[0], fC = hq[2], fB2 = hq[1] + hq[1];
	uint32_t nq0 = 0, nq1 = 0, ne0 = 0, ne1 = 0;
	for (int c = 0; c < 4; ++c) {
		const uint32_t bits = c < 3 ? cb : ab;
		const uint32_t sh = bits ? bits + S : 8u, cmask = bits ? 255u : 0u, qmax = (1u << bits) - 1u;
		const uint32_t qc0 = (f.q0 >> (8*c)) & 255u, qc1 = (f.q1 >> (8*c)) & 255u;
		float dl0[3], dl1[3];
		for (int d = 0; d < 3; ++d) {
			const uint32_t q0 = qc0 + (uint32_t)d - 1u, q1 = qc1 + (uint32_t)d - 1u;   // wraps below zero: > qmax
			const uint32_t d0 = dequant((q0 << S) | P0, sh) & cmask, d1 = dequant((q1 << S) | P1, sh) & cmask;
			dl0[d] = q0 <= qmax ? (float)d0 - xu0[c] : 1.0e18f;
			dl1[d] = q1 <= qmax ? (float)d1 - xu1[c] : 1.0e18f;
		}
		float best = 3.0e38f;
		uint32_t bi = 4u;      // 3 i + j; the centre unless something is better (the centre is always valid)
		for (int i = 0; i < 3; ++i) {
			const float d0 = dl0[i];
			float a0 = fA*d0;
			a0 = a0*d0;
			const float cr = fB2*d0;
			for (int j = 0; j < 3; ++j) {
				const float d1 = dl1[j];
				float v = fC*d1;
				v = fmaf(v, d1, a0);
				v = fmaf(cr, d1, v);
				const bool take = v < best;
				best = take ? v : best;
				bi = take ? (uint32_t)(3*i + j) : bi;
			}
		}
		const uint32_t b0 = bi/3u, b1 = bi - 3u*b0;
		const uint32_t q0 = qc0 + b0 - 1u, q1 = qc1 + b1 - 1u;
		nq0 |= (q0 & 255u) << (8*c);
		nq1 |= (q1 & 255u) << (8*c);
		ne0 |= (dequant((q0 << S) | P0, sh) & cmask) << (8*c);
		ne1 |= (dequant((q1 << S) | P1, sh) & cmask) << (8*c);
	}
	f.q0 = nq0; f.q1 = nq1; f.e0 = ne0; f.e1 = ne1;
}
}
"""

DEVICE_SIDE = r"""
#define __device__
#define __forceinline__ inline
/* Stand-ins for the two instructions, right for what quantize feeds them and for nothing else: finite values (its inputs
   went through clamp255) that are whole numbers (floorf).  They say nothing about the instructions on a NaN or a fraction. */
static inline float __builtin_amdgcn_fmed3f(float a, float b, float c) { return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c)); }
static inline uint32_t __builtin_amdgcn_cvt_pk_u8_f32(float r, uint32_t c, uint32_t w)
{
	const float s = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
	return (w & ~(255u << (8u*c))) | ((uint32_t)rintf(s) << (8u*c));
}
namespace dev {
%s
}
"""

MAIN = r"""
static uint64_t st = 12345;
static uint32_t rnd() { st = st*6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(st >> 32); }
static float rf(float lo, float hi) { return lo + (hi - lo)*(float)(rnd() >> 8)*(1.0f/16777216.0f); }
int main() {
	static const int modes[8][3] = {{4,0,1},{6,0,2},{5,0,0},{7,0,1},{5,6,0},{7,8,0},{7,7,1},{5,5,1}};
	static const int extra[2][3] = {{0,6,0},{0,8,0}};   /* scalar planes of modes 4 / 5 */
	unsigned long n = 0, moved = 0, edge = 0;
	for (int it = 0; it < 1000000; ++it) {
		const int* m = (it % 10) < 8 ? modes[it % 10] : extra[it % 10 - 8];
		const uint32_t cb = m[0], ab = m[1], pbk = m[2];
		uint32_t wt[4] = {6, 13, 2, 1};
		float x0[4], x1[4], u0[4], u1[4];
		const int kind = rnd() % 4;
		for (int c = 0; c < 4; ++c) {
			const bool coded = c < 3 ? cb != 0 : ab != 0;
			float a = kind == 0 ? rf(-40.0f, 295.0f) : (kind == 1 ? (rnd() & 1 ? rf(-3.0f, 6.0f) : rf(249.0f, 258.0f)) : (kind == 2 ? (float)(rnd() % 256) : rf(0.0f, 255.0f)));
			float b = kind == 0 ? rf(-40.0f, 295.0f) : (kind == 1 ? (rnd() & 1 ? rf(-3.0f, 6.0f) : rf(249.0f, 258.0f)) : (kind == 2 ? (float)(rnd() % 256) : rf(0.0f, 255.0f)));
			u0[c] = coded ? a : 0.0f; u1[c] = coded ? b : 0.0f;
			x0[c] = u0[c] < 0.0f ? 0.0f : (u0[c] > 255.0f ? 255.0f : u0[c]);
			x1[c] = u1[c] < 0.0f ? 0.0f : (u1[c] > 255.0f ? 255.0f : u1[c]);
		}
		SubFit a, b;
		memset(&a, 0, sizeof a); memset(&b, 0, sizeof b);
		if (it & 1) { ref::quantize<true>(x0, x1, cb, ab, pbk, wt, a); dev::quantize<true>(x0, x1, cb, ab, pbk, wt, b); }
		else { ref::quantize<false>(x0, x1, cb, ab, pbk, wt, a); dev::quantize<false>(x0, x1, cb, ab, pbk, wt, b); }
		if (memcmp(&a, &b, sizeof a)) { printf("quantize differs it %d cb %u ab %u pbk %u: %08x %08x %08x %08x %u | %08x %08x %08x %08x %u\n", it, cb, ab, pbk, a.q0, a.q1, a.e0, a.e1, a.pb, b.q0, b.q1, b.e0, b.e1, b.pb); return 1; }
		/* the window: sums of a real selector set (weights of a 2..4-bit index on n texels) */
		int nn = 1 + rnd() % 16, ib = 2 + rnd() % 3, S = 0, A = 0, B = 0, C = 0;
		for (int i = 0; i < nn; ++i) { int k = rnd() % (1 << ib), d = (1 << ib) - 1, w = (k*64 + d/2)/d, iw = 64 - w; S += w; A += iw*iw; B += iw*w; C += w*w; }
		if (nn*C - S*S <= 0) continue;
		float hq[3] = {(float)A, (float)B, (float)C};
		const SubFit before = a;
		ref::refit_window(u0, u1, hq, cb, ab, pbk, a);
		dev::refit_window(u0, u1, hq, cb, ab, pbk, b);
		if (memcmp(&a, &b, sizeof a)) { printf("refit_window differs it %d cb %u ab %u pbk %u: %08x %08x %08x %08x | %08x %08x %08x %08x (from %08x %08x)\n", it, cb, ab, pbk, a.q0, a.q1, a.e0, a.e1, b.q0, b.q1, b.e0, b.e1, before.q0, before.q1); return 1; }
		++n;
		moved += a.q0 != before.q0 || a.q1 != before.q1;
		for (int c = 0; c < 4; ++c) { uint32_t bits = c < 3 ? cb : ab, qm = (1u << bits) - 1u, v = (before.q0 >> (8*c)) & 255u; if (bits && (v == 0 || v == qm)) { ++edge; break; } }
	}
	printf("equal on %lu cases, window moved %lu, field of end nought at a range end %lu\n", n, moved, edge);
	return 0;
}
"""


def _cut(text, start, end):
    """The source from the line that opens a function to the comment that follows it in bc7_encode.hip"""
    a = text.find(start)
    assert a >= 0, "bc7_encode.hip no longer has the line %r: point this test at the function's new opening line" % start
    b = text.find(end, a)
    assert b >= 0, "bc7_encode.hip no longer has the comment %r after %r: point this test at what follows the function now" % (end, start)
    return text[a:b]


def test_whole_word_forms_equal_the_per_channel_forms(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler is needed"
    hip = open(os.path.join(CSRC, "bc7_encode.hip")).read()
    dev = _cut(hip, "template <bool UNITW>\n__device__ __forceinline__ void quantize(", "// View of one block's texels in LDS") + \
        _cut(hip, "__device__ __forceinline__ void refit_window(", "// Fit-geometry cache")
    src = tmp_path / "twin.cpp"
    src.write_text(PRELUDE + REFERENCE + DEVICE_SIDE % dev + MAIN)
    exe = tmp_path / "twin"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    compared, moved, at_end = (int(v) for v in re.findall(r"\d+", run.stdout)[:3])
    assert compared > 900000 and moved > 100000 and at_end > 100000, run.stdout
