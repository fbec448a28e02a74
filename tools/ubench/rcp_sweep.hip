// Sweep behind csrc/bc7_rcp.h: v_rcp_f32 and one Newton step against the compiler's 1.0f/x on every float with the sign
// bit clear.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o rcp_sweep.bin rcp_sweep.hip ; run on the GPU box.
// Prints, for the patterns bc7_rcp.h admits (biased exponent 2..252) and for the rest, how many there are and on how
// many the step, and v_rcp_f32 alone, differ from the quotient.  Exit status 1 when an admitted pattern differs.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "../../cuttlefish_amd/csrc/bc7_rcp.h"

// cnt: [0] admitted, [1] admitted and the step differs, [2] admitted and v_rcp_f32 alone differs,
//      [3] not admitted, [4] not admitted and the step differs, [5] lowest admitted pattern that differs
__global__ void __launch_bounds__(256) sweep(unsigned long long* cnt)
{
	const uint64_t stride = (uint64_t)gridDim.x*blockDim.x;
	unsigned long long c[5] = {0, 0, 0, 0, 0}, first = ~0ull;
	for (uint64_t p = (uint64_t)blockIdx.x*blockDim.x + threadIdx.x; p < (1ull << 31); p += stride) {
		const float x = __uint_as_float((uint32_t)p);
		const float q = 1.0f/x;
		const float s = cf_rcp_ranged(x);
		const float r = __builtin_amdgcn_rcpf(x);
		const bool ds = __float_as_uint(q) != __float_as_uint(s), dr = __float_as_uint(q) != __float_as_uint(r);
		if (cf_rcp_admits(x)) {
			c[0] += 1; c[1] += ds; c[2] += dr;
			if (ds && p < first) first = p;
		} else {
			c[3] += 1; c[4] += ds;
		}
	}
	for (int i = 0; i < 5; ++i)
		atomicAdd(&cnt[i], c[i]);
	atomicMin(&cnt[5], first);
}

int main()
{
	unsigned long long* d;
	unsigned long long h[6] = {0, 0, 0, 0, 0, ~0ull};
	if (hipMalloc(&d, sizeof h) != hipSuccess) return 2;
	(void)hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice);
	hipLaunchKernelGGL(sweep, dim3(4096), dim3(256), 0, 0, d);
	if (hipDeviceSynchronize() != hipSuccess) return 2;
	(void)hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
	printf("admitted (biased exponent 2..252): %llu patterns, step differs on %llu, v_rcp_f32 alone on %llu\n", h[0], h[1], h[2]);
	printf("not admitted: %llu patterns, step differs on %llu\n", h[3], h[4]);
	if (h[1]) printf("lowest admitted pattern that differs: 0x%08llx\n", h[5]);
	(void)hipFree(d);
	return h[1] ? 1 : 0;
}
