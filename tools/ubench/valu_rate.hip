// Micro-benchmark: VALU issue rate of gfx950 per instruction (wave64), one opcode at a time.
// Build: hipcc --offload-arch=gfx950 -O3 -o valu_rate.bin valu_rate.hip ; run on the GPU box.
// Each wave runs ITER iterations of 16 independent dependency chains of ONE instruction
// (inline asm, so the compiler can neither fold nor re-associate it); the grid puts WAVES
// waves on every SIMD of every CU.  Reported: ns per wave-instruction per SIMD at the highest
// occupancy (= issue throughput) and the same in cycles at 2.4 GHz.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

#define ITER 2048

#define BODY(ASMSTR, CONSTR_EXTRA)                                                        \
	for (int it = 0; it < ITER; ++it) {                                                   \
		_Pragma("unroll") for (int i = 0; i < 16; ++i)                                    \
			asm volatile(ASMSTR : "+v"(a[i]) : "v"(b), "v"(c) CONSTR_EXTRA);              \
	}

template <int OP>
__global__ void __launch_bounds__(256) k(uint32_t* out, uint32_t seed)
{
	uint32_t a[16];
#pragma unroll
	for (int i = 0; i < 16; ++i) a[i] = seed + threadIdx.x*17u + i;
	uint32_t b = seed*3u + 1u + threadIdx.x, c = seed ^ 0x5bd1e995u;
	if (OP == 0) BODY("v_add_u32 %0, %0, %1", )
	if (OP == 1) BODY("v_fma_f32 %0, %0, %1, %2", )
	if (OP == 2) BODY("v_dot4_u32_u8 %0, %0, %1, %2", )
	if (OP == 3) BODY("v_lshlrev_b32 %0, 3, %0", )
	if (OP == 4) BODY("v_lshl_add_u32 %0, %0, 8, %1", )
	if (OP == 5) BODY("v_and_b32 %0, %0, %1", )
	if (OP == 6) BODY("v_max3_i32 %0, %0, %1, %2", )
	if (OP == 7) BODY("v_mul_u32_u24 %0, %0, %1", )
	if (OP == 8) BODY("v_mad_u32_u24 %0, %0, %1, %2", )
	if (OP == 9) BODY("v_mul_lo_u32 %0, %0, %1", )
	if (OP == 10) BODY("v_cvt_f32_u32 %0, %0", )
	if (OP == 11) BODY("v_floor_f32 %0, %0", )
	if (OP == 12) BODY("v_perm_b32 %0, %0, %1, %2", )
	if (OP == 13) BODY("v_cndmask_b32 %0, %0, %1, vcc", )
	if (OP == 14) BODY("v_mov_b32_dpp %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf", )
	if (OP == 15) BODY("v_mul_f32 %0, %0, %1", )
	if (OP == 16) BODY("v_add_f32 %0, %0, %1", )
	if (OP == 17) BODY("v_bfe_u32 %0, %0, 8, 8", )
	if (OP == 18) BODY("v_min_u32 %0, %0, %1", )
	if (OP == 19) BODY("v_cvt_f32_ubyte0 %0, %0", )
	if (OP == 20) BODY("v_sub_u32 %0, %1, %0", )
	if (OP == 21) BODY("v_lshl_or_b32 %0, %0, 8, %1", )
	if (OP == 22) BODY("v_add3_u32 %0, %0, %1, %2", )
	if (OP == 23) BODY("v_mad_i32_i24 %0, %0, %1, %2", )
	if (OP == 24) BODY("v_mul_i32_i24 %0, %0, %1", )
	if (OP == 25) BODY("v_sad_u8 %0, %0, %1, %2", )
	if (OP == 26) BODY("v_med3_i32 %0, %0, %1, %2", )
	if (OP == 27) BODY("v_ashrrev_i32 %0, 3, %0", )
	if (OP == 28) {   // 64-bit accumulate: the destination is a register pair
		unsigned long long acc[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) acc[i] = a[i];
		for (int it = 0; it < ITER; ++it) {
#pragma unroll
			for (int rep = 0; rep < 2; ++rep)
#pragma unroll
				for (int i = 0; i < 8; ++i)
					asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[i]) : "v"(b), "v"(c) : "vcc");
		}
#pragma unroll
		for (int i = 0; i < 8; ++i) a[i] = (uint32_t)acc[i] ^ (uint32_t)(acc[i] >> 32);
	}
	if (OP >= 29 && OP <= 31) {   // packed fp32: both operands and the destination are register pairs (two floats per lane)
		unsigned long long acc[8];
		const unsigned long long b2 = ((unsigned long long)__float_as_uint(1.0f + (float)(b & 255u)/1024.0f) << 32) | __float_as_uint(0.999f);
		const unsigned long long c2 = ((unsigned long long)__float_as_uint(0.25f) << 32) | __float_as_uint((float)(c & 15u));
#pragma unroll
		for (int i = 0; i < 8; ++i)
			acc[i] = ((unsigned long long)__float_as_uint((float)a[i]) << 32) | __float_as_uint((float)a[i + 8]);
		for (int it = 0; it < ITER; ++it) {
#pragma unroll
			for (int rep = 0; rep < 2; ++rep)
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					if (OP == 29) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(acc[i]) : "v"(b2), "v"(c2));
					if (OP == 30) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(acc[i]) : "v"(b2), "v"(c2));
					if (OP == 31) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(acc[i]) : "v"(b2), "v"(c2));
				}
		}
#pragma unroll
		for (int i = 0; i < 8; ++i) a[i] = (uint32_t)acc[i] ^ (uint32_t)(acc[i] >> 32);
	}
	if (OP == 32) {   // what a scalar-spill reload is: one lane of a vector register to a scalar register
		uint32_t s[16];
		for (int it = 0; it < ITER; ++it) {
#pragma unroll
			for (int i = 0; i < 16; ++i)
				asm volatile("v_readlane_b32 %0, %1, 5" : "=s"(s[i]) : "v"(a[i]));
		}
#pragma unroll
		for (int i = 0; i < 16; ++i) a[i] ^= s[i];
	}
	if (OP == 33) {   // ... and the spill itself: a scalar into one lane
		const uint32_t sv = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
		for (int it = 0; it < ITER; ++it) {
#pragma unroll
			for (int i = 0; i < 16; ++i)
				asm volatile("v_writelane_b32 %0, %1, 5" : "+v"(a[i]) : "s"(sv));
		}
	}
	// a select behind the compare that produces its mask (the v_cndmask_b32 row above reads a VCC nobody wrote and is not
	// representative): two instructions per chain step, reported per instruction
	if (OP == 34) BODY("v_cmp_lt_u32 vcc, %1, %0\n\tv_cndmask_b32 %0, %0, %2, vcc", : "vcc")
	if (OP == 35) BODY("v_cmp_lt_u32 vcc, %1, %0", : "vcc")   // the compare alone
	// the classes the bookkeeping of the BC7 selector search and its reciprocals are made of, and the two fp16 dot
	// products a float-keyed search would issue per (texel, palette entry)
	if (OP == 36) BODY("v_alignbit_b32 %0, %0, %1, 8", )
	if (OP == 37) BODY("v_lshrrev_b32 %0, 3, %0", )
	if (OP == 38) BODY("v_bfe_i32 %0, %0, 7, 25", )
	if (OP == 39) BODY("v_and_or_b32 %0, %0, %1, %2", )
	if (OP == 40) BODY("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96", )
	if (OP == 41) BODY("v_max_f32 %0, %0, %1", )
	if (OP == 42) BODY("v_max3_f32 %0, %0, %1, %2", )
	if (OP == 43) BODY("v_rcp_f32 %0, %0", )
	if (OP == 44) BODY("v_cvt_i32_f32 %0, %0", )
	if (OP == 45) BODY("v_dot2_f32_f16 %0, %1, %2, %0", )
	if (OP == 46) BODY("v_dot2c_f32_f16 %0, %1, %2", )
	// the minimum-form key of the BC7 selector search (multiply-add with the factor in a scalar register, as the kernel
	// holds its -256; v_min3_i32) and the refit window's row minima
	if (OP == 47) BODY("v_min3_i32 %0, %0, %1, %2", )
	if (OP == 48) BODY("v_min3_f32 %0, %0, %1, %2", )
	if (OP == 49) {
		int sm = -256;
		asm volatile("" : "+s"(sm));
		for (int it = 0; it < ITER; ++it) {
#pragma unroll
			for (int i = 0; i < 16; ++i)
				asm volatile("v_mad_i32_i24 %0, %0, %1, %2" : "+v"(a[i]) : "s"(sm), "v"(c));
		}
	}
	uint32_t r = 0;
#pragma unroll
	for (int i = 0; i < 16; ++i) r ^= a[i];
	out[blockIdx.x*blockDim.x + threadIdx.x] = r;
}

// The matrix pipe beside the vector pipe: v_mfma_i32_4x4x4_16b_i8 (16 batches of 4x4x4 int8, cbsz:3 as the BC7 selector
// search would issue it), four per loop trip, with FILL independent v_mad_i32_i24 / v_min3_i32 (alternating) behind
// every MFMA and, with READ, four v_mad_i32_i24 that read its four result registers.  Builtins and plain C++ here, not
// inline asm: the compiler then places the wait states an MFMA's result needs, as it would in the kernel (s_nop 4
// between an MFMA and the first reader of its result, s_nop 0 between a vector instruction and the MFMA behind it).
// A "group" in the output is one MFMA with its fillers and readers.
typedef int cf_i4 __attribute__((ext_vector_type(4)));
#define MFMA_ITER 1024

template <int FILL, bool READ>
__global__ void __launch_bounds__(256, 4) kmfma(uint32_t* out, uint32_t seed)
{
	cf_i4 acc[4];
	int f[12], rd[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) acc[i] = cf_i4{(int)seed + i, (int)threadIdx.x, i, 1};
#pragma unroll
	for (int i = 0; i < 12; ++i) f[i] = (int)(seed*7u + threadIdx.x + i);
#pragma unroll
	for (int i = 0; i < 4; ++i) rd[i] = i;
	int a = (int)(seed*3u + 1u + threadIdx.x), b = (int)(seed ^ 0x5bd1e995u ^ threadIdx.x), c = (int)(seed & 0xFFFFu);
	int sm = -256;
	asm volatile("" : "+s"(sm), "+v"(a), "+v"(b), "+v"(c));
	cf_i4 c0 = acc[0];
	asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z), "+v"(c0.w));
	for (int it = 0; it < MFMA_ITER; ++it) {
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			// C is not carried round the loop (the kernel's is a fresh operand per row), and the result is pinned to
			// vector registers as the kernel holds it: an accumulation chain would be moved to the AGPR file
			asm volatile("" : "+v"(a));   // (opaque per issue: the product is not loop-invariant to the compiler)
			acc[i] = __builtin_amdgcn_mfma_i32_4x4x4i8(a, b, c0, 3, 0, 0);
			asm volatile("" : "+v"(acc[i]));
#pragma unroll
			for (int j = 0; j < FILL; ++j) {
				if (j & 1) { const int m = f[j] < b ? f[j] : b; f[j] = m < c ? m : c; }
				else f[j] = __mul24(f[j], sm) + c;
				asm volatile("" : "+v"(f[j]));
			}
			if (READ) {
				rd[0] = __mul24(acc[i].x, sm) + rd[0]; rd[1] = __mul24(acc[i].y, sm) + rd[1];
				rd[2] = __mul24(acc[i].z, sm) + rd[2]; rd[3] = __mul24(acc[i].w, sm) + rd[3];
				asm volatile("" : "+v"(rd[0]), "+v"(rd[1]), "+v"(rd[2]), "+v"(rd[3]));
			}
		}
	}
	int r = 0;
#pragma unroll
	for (int i = 0; i < 4; ++i) r ^= acc[i].x ^ acc[i].y ^ acc[i].z ^ acc[i].w ^ rd[i];
#pragma unroll
	for (int i = 0; i < 12; ++i) r ^= f[i];
	out[blockIdx.x*blockDim.x + threadIdx.x] = (uint32_t)r;
}

template <int FILL, bool READ>
static void run_mfma(int waves_per_simd)
{
	int ncu = 0;
	(void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
	const int blocks = ncu*waves_per_simd;
	uint32_t* out;
	(void)hipMalloc(&out, (size_t)blocks*256*4);
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
	hipLaunchKernelGGL((kmfma<FILL, READ>), dim3(blocks), dim3(256), 0, 0, out, 12345u);
	(void)hipDeviceSynchronize();
	(void)hipEventRecord(e0);
	for (int rep = 0; rep < 5; ++rep)
		hipLaunchKernelGGL((kmfma<FILL, READ>), dim3(blocks), dim3(256), 0, 0, out, 12345u);
	(void)hipEventRecord(e1);
	(void)hipEventSynchronize(e1);
	float ms; (void)hipEventElapsedTime(&ms, e0, e1);
	ms /= 5.0f;
	const double groups = (double)MFMA_ITER*4*waves_per_simd;   // (MFMA + its fillers and readers) per SIMD
	const double ns = ms*1e6/groups;
	printf("mfma_i32_4x4x4_i8 + %2d fill + %d readers  waves/SIMD %d  %7.3f ms  %6.2f ns/group/SIMD  = %5.2f cycles @2.4GHz\n",
		FILL, READ ? 4 : 0, waves_per_simd, ms, ns, ns*2.4);
	(void)hipFree(out);
}

template <int OP>
static void run(const char* name, int waves_per_simd, int per_step = 1)   // per_step: instructions per chain step
{
	int ncu = 0;
	(void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
	const int blocks = ncu*waves_per_simd;   // 256 threads = 4 waves = one per SIMD
	uint32_t* out;
	(void)hipMalloc(&out, (size_t)blocks*256*4);
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
	hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(256), 0, 0, out, 12345u);
	(void)hipDeviceSynchronize();
	(void)hipEventRecord(e0);
	for (int rep = 0; rep < 5; ++rep)
		hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(256), 0, 0, out, 12345u);
	(void)hipEventRecord(e1);
	(void)hipEventSynchronize(e1);
	float ms; (void)hipEventElapsedTime(&ms, e0, e1);
	ms /= 5.0f;
	const double instr = (double)ITER*16*waves_per_simd*per_step;   // wave-instructions per SIMD
	const double ns = ms*1e6/instr;
	printf("%-18s waves/SIMD %d  %7.3f ms  %5.2f ns/wave-instr/SIMD  = %4.2f cycles @2.4GHz\n",
		name, waves_per_simd, ms, ns, ns*2.4);
	(void)hipFree(out);
}

int main(int argc, char** argv)
{
	// "mfma" as the argument: the matrix-pipe rows alone, with the three vector rows they are compared with
	const bool only_mfma = argc > 1 && argv[1][0] == 'm';
	for (int w : {4, 8}) {
		if (only_mfma) { run<2>("v_dot4_u32_u8", w);   run<49>("v_mad_i32_i24 sgpr", w);   run<12>("v_perm_b32", w); }
		run_mfma<0, false>(w);  run_mfma<4, false>(w);  run_mfma<8, false>(w);  run_mfma<12, false>(w);
		run_mfma<0, true>(w);   run_mfma<4, true>(w);   run_mfma<8, true>(w);   run_mfma<12, true>(w);
	}
	if (only_mfma)
		return 0;
	for (int w : {4, 8}) {
		run<0>("v_add_u32", w);       run<20>("v_sub_u32", w);     run<22>("v_add3_u32", w);
		run<5>("v_and_b32", w);       run<3>("v_lshlrev_b32", w);  run<4>("v_lshl_add_u32", w);
		run<21>("v_lshl_or_b32", w);  run<17>("v_bfe_u32", w);     run<12>("v_perm_b32", w);
		run<18>("v_min_u32", w);      run<6>("v_max3_i32", w);     run<13>("v_cndmask_b32", w);
		run<7>("v_mul_u32_u24", w);   run<8>("v_mad_u32_u24", w);  run<9>("v_mul_lo_u32", w);
		run<2>("v_dot4_u32_u8", w);   run<14>("v_mov_b32_dpp", w);
		run<10>("v_cvt_f32_u32", w);  run<19>("v_cvt_f32_ubyte0", w); run<11>("v_floor_f32", w);
		run<1>("v_fma_f32", w);       run<15>("v_mul_f32", w);     run<16>("v_add_f32", w);
		run<23>("v_mad_i32_i24", w);  run<24>("v_mul_i32_i24", w); run<25>("v_sad_u8", w);
		run<26>("v_med3_i32", w);     run<27>("v_ashrrev_i32", w); run<28>("v_mad_u64_u32", w);
		run<29>("v_pk_mul_f32", w);   run<30>("v_pk_add_f32", w);  run<31>("v_pk_fma_f32", w);
		run<32>("v_readlane_b32", w); run<33>("v_writelane_b32", w);
		run<35>("v_cmp_lt_u32", w);   run<34>("v_cmp+v_cndmask", w, 2);
		run<36>("v_alignbit_b32", w); run<37>("v_lshrrev_b32", w); run<38>("v_bfe_i32", w);
		run<39>("v_and_or_b32", w);   run<40>("v_bitop3_b32", w);
		run<41>("v_max_f32", w);      run<42>("v_max3_f32", w);
		run<43>("v_rcp_f32", w);      run<44>("v_cvt_i32_f32", w);
		run<45>("v_dot2_f32_f16", w); run<46>("v_dot2c_f32_f16", w);
		run<47>("v_min3_i32", w);     run<48>("v_min3_f32", w);    run<49>("v_mad_i32_i24 sgpr", w);
	}
	return 0;
}
