// 1.0f/x of bc7_encode.hip without the division's expansion, where the argument's range is known.
//
// The compiler expands a float division to v_div_scale x 2, v_rcp_f32, four v_fma, v_div_fmas and v_div_fixup.
// v_rcp_f32 followed by one Newton step, e = fma(-x, r, 1), r' = fma(e, r, r), returns the correctly rounded quotient --
// the division's float -- for EVERY positive x whose biased exponent lies in 2..252: tools/ubench/rcp_sweep.hip compares
// the two on all 251 * 2^23 such bit patterns on the device (v_rcp_f32 alone differs on about a tenth of them).  Outside
// that range (zero, denormals, the two smallest and the two largest binades, infinity, NaN) the step can differ, and a
// negative x is not swept: such arguments keep the division.
//
// Ranges by construction (cf_rcp_ranged, no test in front; checked numerically by tests/test_bc7_rcp_ranges.py):
//   1/(64 det)    det = n C - S^2 as an integer, replaced by 1 when it is not positive; n <= 16 texels, C <= 16 * 64^2:
//                 64 <= 64 det <= 2^26, biased exponent 133..153.
//   1/sqrt(l2)    l2 = sum of the squares of an axis divided by its largest magnitude mx > 0: the largest component
//   1/den         is mx * (1/mx) = 1 to within one rounding of each operation, every other one is at most that, so
//                 1 - 2^-21 < l2 < 4 + 2^-20 and sqrt(l2) lies in [1 - 2^-21, 2 + 2^-20]: biased exponent 126..129
//                 (den is the same sum).  This needs 1/mx to be finite and normal, which the test below gives: the
//                 covariance terms are integers below 2^24 as floats, a power-iteration step multiplies by at most
//                 4 * 2^24, and sums of integers round to integers, so a positive mx lies in [1, 2^102].
// Behind a test of the exponent (cf_rcp_tested): 1/mx, the largest magnitude after the power iteration.  By the bound
// above the test always passes; it is kept because that bound leans on the iteration count, and a change there should
// cost a branch, not a wrong block.
#ifndef CFHIP_BC7_RCP_H
#define CFHIP_BC7_RCP_H

#include <stdint.h>

#if defined(__HIPCC__)
__device__ __forceinline__ float cf_rcp_ranged(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	float r = __builtin_amdgcn_rcpf(x);
	const float e = __builtin_fmaf(-x, r, 1.0f);
	r = __builtin_fmaf(e, r, r);
	return r;
#else
	return 1.0f/x;     // (the host pass of a device function: never called)
#endif
}
__device__ __forceinline__ bool cf_rcp_admits(float x)
{
	// sign clear and biased exponent in 2..252
	return (__float_as_uint(x) >> 23) - 2u <= 250u;
}
__device__ __forceinline__ float cf_rcp_tested(float x)
{
	return cf_rcp_admits(x) ? cf_rcp_ranged(x) : 1.0f/x;
}
#endif

#endif
