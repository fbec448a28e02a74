// Operand layout of v_mfma_i32_4x4x4_16b_i8 as a BC7 selector search on the matrix pipe would rely on it (DESIGN.md
// section 4.1, tenth step: texels of a block row as A, one palette entry per lane as B).
// Build: hipcc --offload-arch=gfx950 -O3 -o mfma_layout.bin mfma_layout.hip ; run on the GPU box.
// One wavefront.  Every lane supplies four seeded signed bytes of A, four of B and four words of C; the host forms
// what the layout below says every lane must receive and compares all 64 x 4 results, for cbsz 0, 3 and 4:
//   lane 4b + i holds row i of batch b's A (bytes k = 0..3) and column i of batch b's B (bytes k = 0..3);
//   lane 4b + j receives D[b][i][j] = C[b][i][j] + sum_k A[b'][i][k] B[b][k][j] in register i, where b' = b without
//   broadcast (cbsz 0), the first batch of b's group of eight (cbsz 3: one A block per half-wavefront) or batch 0
//   (cbsz 4: one A block per wavefront).
// Prints one line per form; exit status 1 when a lane differs from this layout.
// A last line records what the hardware does under a partial execution mask (probe_masked below): how many results of
// the issuing lanes still equal the full-mask ones, and whether the switched-off lanes kept their registers.  Only the
// second is checked (exit status 1 when a switched-off lane's value changed): on gfx950 all 224 results differ, which
// is why a kernel must issue the instruction with the lanes that hold its A rows switched on.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

typedef int cf_i4 __attribute__((ext_vector_type(4)));

template <int CBSZ>
__global__ void __launch_bounds__(64) probe(const int* a, const int* b, const cf_i4* c, cf_i4* d)
{
	const uint32_t l = threadIdx.x;
	d[l] = __builtin_amdgcn_mfma_i32_4x4x4i8(a[l], b[l], c[l], CBSZ, 0, 0);
}

// The same under a partial execution mask, as a fit under a divergent branch would issue it: A, B and C are loaded by every lane, then only the
// lanes >= 8 issue the instruction (cbsz:4, so every batch reads the A rows of lanes 0..3, which are switched off).
__global__ void __launch_bounds__(64) probe_masked(const int* a, const int* b, const cf_i4* c, cf_i4* d)
{
	const uint32_t l = threadIdx.x;
	const int av = a[l], bv = b[l];
	const cf_i4 cv = c[l];
	cf_i4 r = {0x5EED, 0x5EED, 0x5EED, 0x5EED};
	if (l >= 8u)
		r = __builtin_amdgcn_mfma_i32_4x4x4i8(av, bv, cv, 4, 0, 0);
	d[l] = r;
}

static int sbyte(int w, int k) { return (int)(int8_t)((uint32_t)w >> (8*k)); }

template <int CBSZ>
static int check(const int* ha, const int* hb, const int (*hc)[4], const int* da, const int* db, const cf_i4* dc, cf_i4* dd)
{
	int hd[64][4];
	hipLaunchKernelGGL(probe<CBSZ>, dim3(1), dim3(64), 0, 0, da, db, dc, dd);
	if (hipDeviceSynchronize() != hipSuccess) return -1;
	(void)hipMemcpy(hd, dd, sizeof hd, hipMemcpyDeviceToHost);
	int bad = 0, first = -1;
	for (int l = 0; l < 64; ++l) {
		const int b = l >> 2, j = l & 3;
		const int ab = CBSZ == 0 ? b : (CBSZ == 3 ? (b & ~7) : 0);
		for (int i = 0; i < 4; ++i) {
			int want = hc[l][i];
			for (int k = 0; k < 4; ++k)
				want += sbyte(ha[4*ab + i], k)*sbyte(hb[4*b + j], k);
			if (want != hd[l][i]) { ++bad; if (first < 0) first = l; }
		}
	}
	if (bad)
		printf("cbsz:%d  %d of 256 results differ from the host's, first in lane %d\n", CBSZ, bad, first);
	else
		printf("cbsz:%d  all 64 lanes x 4 results equal the host's\n", CBSZ);
	return bad;
}

int main()
{
	int ha[64], hb[64], hc[64][4];
	uint32_t s = 0x9E3779B9u;
	auto next = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
	for (int l = 0; l < 64; ++l) {
		ha[l] = (int)next(); hb[l] = (int)next();
		for (int i = 0; i < 4; ++i) hc[l][i] = (int)(next() >> 8) - (1 << 23);
	}
	// the sign boundary and the extremes in the lanes every form reads
	ha[0] = (int)0x807F00FFu; hb[1] = (int)0x7F80FF00u; ha[33] = (int)0x80808080u; hb[34] = (int)0x7F7F7F7Fu;
	int *da, *db; cf_i4 *dc, *dd;
	if (hipMalloc(&da, sizeof ha) != hipSuccess || hipMalloc(&db, sizeof hb) != hipSuccess ||
		hipMalloc(&dc, sizeof hc) != hipSuccess || hipMalloc(&dd, sizeof hc) != hipSuccess) return 2;
	(void)hipMemcpy(da, ha, sizeof ha, hipMemcpyHostToDevice);
	(void)hipMemcpy(db, hb, sizeof hb, hipMemcpyHostToDevice);
	(void)hipMemcpy(dc, hc, sizeof hc, hipMemcpyHostToDevice);
	const int r0 = check<0>(ha, hb, hc, da, db, dc, dd);
	const int r3 = check<3>(ha, hb, hc, da, db, dc, dd);
	const int r4 = check<4>(ha, hb, hc, da, db, dc, dd);
	// partial execution mask: recorded, see the header; the lanes that are off must keep their own value
	int hm[64][4], badm = 0, kept = 0;
	hipLaunchKernelGGL(probe_masked, dim3(1), dim3(64), 0, 0, da, db, dc, dd);
	if (hipDeviceSynchronize() != hipSuccess) return 2;
	(void)hipMemcpy(hm, dd, sizeof hm, hipMemcpyDeviceToHost);
	for (int l = 0; l < 64; ++l)
		for (int i = 0; i < 4; ++i) {
			int want = hc[l][i];
			for (int k = 0; k < 4; ++k)
				want += sbyte(ha[i], k)*sbyte(hb[l], k);
			if (l >= 8) badm += want != hm[l][i];
			else kept += hm[l][i] == 0x5EED;
		}
	printf("cbsz:4 issued by lanes 8..63 only: %d of 224 results differ from the host's (A rows from the switched-off lanes 0..3); "
		"%d of 32 values of lanes 0..7 kept\n", badm, kept);
	const int lost = kept != 32;
	(void)hipFree(da); (void)hipFree(db); (void)hipFree(dc); (void)hipFree(dd);
	if (r0 < 0 || r3 < 0 || r4 < 0) return 2;
	return (r0 | r3 | r4 | lost) ? 1 : 0;
}
