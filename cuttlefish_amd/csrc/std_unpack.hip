// std_unpack.hip -- the payload of an uncompressed ("standard") format back to RGBA32F texels on gfx950: the
// inverse of std_pack.hip, field for field.
//
// Like the packer this is an HBM-bound kernel, and the store-heavy direction of the two: 1..16 B read and 16 B
// written per pixel.  Its shape mirrors the packer's:
//   * one workgroup = 512 consecutive pixels of the linear index; a lane holds two pixels 256 apart, so every
//     wave-level store is one contiguous 1 KB run of whole float4 texels (dwordx4 per lane);
//   * payload and texels are touched once: loads and stores are nontemporal;
//   * pixels of 4 / 8 / 12 / 16 bytes are loaded straight into registers as dword .. dwordx4;
//   * pixels of 1 / 2 / 3 / 6 bytes would be one to three sub-dword loads per lane: the workgroup's contiguous
//     payload run is read as aligned dwords into LDS instead (at most 3 KB), and each lane picks its bytes from
//     there with one v_alignbyte per dword.  The run may start at any byte: the partial dwords at its two ends
//     are read byte by byte, so nothing outside the payload is touched;
//   * the conversion is a wave-uniform runtime switch: one kernel per pixel size;
//   * the payload is tight (width*height pixels); the output has a row pitch.
// No scratch, no spilled VGPR, no AGPR (cuttlefish_amd/build.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "std_unpack.h"

namespace {

using namespace cfstd;

struct unpack_args {
	const uint8_t* pixels;
	uint8_t* out;
	unsigned long long out_pitch;
	uint32_t width, height;
	uint32_t format, type;
	uint32_t in_vec;              // pixels is aligned for the vector load of its pixel size
	uint32_t out_vec;             // out and out_pitch are 16-byte aligned
};

template <int BPP>
__global__ __launch_bounds__(kThreads) void cfhip_std_unpack_kernel(const unpack_args a)
{
	__shared__ uint32_t stage[stage_dwords<BPP>()];
	const uint32_t tid = threadIdx.x;
	const unsigned long long npix = (unsigned long long)a.width*a.height;
	const unsigned long long p0 = (unsigned long long)blockIdx.x*kPixPerWg;
	const bool tight = a.out_pitch == (unsigned long long)a.width*16u;
	uint4 o[kPerThread];
	load_pixels<BPP>(a.pixels, a.in_vec, p0, npix, tid, stage, o);
#pragma unroll
	for (uint32_t j = 0; j < kPerThread; ++j) {
		const unsigned long long p = p0 + j*kThreads + tid;
		if (p >= npix)
			continue;
		const float4 f = unpack_pixel<BPP>(a.format, a.type, o[j]);
		unsigned long long off;
		if (tight)
			off = p*16u;
		else {
			const uint32_t y = (uint32_t)(p/a.width);
			const uint32_t x = (uint32_t)(p - (unsigned long long)y*a.width);
			off = (unsigned long long)y*a.out_pitch + (unsigned long long)x*16u;
		}
		if (a.out_vec) {
			typedef float f4v __attribute__((ext_vector_type(4)));
			const f4v v = {f.x, f.y, f.z, f.w};
			__builtin_nontemporal_store(v, reinterpret_cast<f4v*>(a.out + off));
		} else {
			float* d = reinterpret_cast<float*>(a.out + off);
			d[0] = f.x; d[1] = f.y; d[2] = f.z; d[3] = f.w;
		}
	}
}

} // namespace

// format: Texture::Format 1..28, type: Texture::Type, a legal pair of bytes_per_pixel bytes.  pixels: the tight
// payload, any alignment; out: rows out_pitch bytes apart, 4-byte aligned (16 for the float4 stores).
extern "C" hipError_t cfhip_launch_std_unpack(int format, int type, int bytes_per_pixel, const void* pixels,
	uint32_t width, uint32_t height, void* out, size_t out_pitch, hipStream_t stream)
{
	unpack_args a;
	a.pixels = static_cast<const uint8_t*>(pixels);
	a.out = static_cast<uint8_t*>(out);
	a.out_pitch = out_pitch;
	a.width = width; a.height = height;
	a.format = (uint32_t)format; a.type = (uint32_t)type;
	const uintptr_t al = bytes_per_pixel == 16 ? 16u : (bytes_per_pixel == 8 ? 8u : 4u);
	a.in_vec = (uintptr_t)pixels % al == 0 ? 1u : 0u;
	a.out_vec = ((uintptr_t)out % 16u == 0 && out_pitch % 16u == 0) ? 1u : 0u;
	const unsigned long long npix = (unsigned long long)width*height;
	const dim3 grid((unsigned)((npix + kPixPerWg - 1)/kPixPerWg)), block(kThreads);
	switch (bytes_per_pixel) {
		case 1: hipLaunchKernelGGL(cfhip_std_unpack_kernel<1>, grid, block, 0, stream, a); break;
		case 2: hipLaunchKernelGGL(cfhip_std_unpack_kernel<2>, grid, block, 0, stream, a); break;
		case 3: hipLaunchKernelGGL(cfhip_std_unpack_kernel<3>, grid, block, 0, stream, a); break;
		case 4: hipLaunchKernelGGL(cfhip_std_unpack_kernel<4>, grid, block, 0, stream, a); break;
		case 6: hipLaunchKernelGGL(cfhip_std_unpack_kernel<6>, grid, block, 0, stream, a); break;
		case 8: hipLaunchKernelGGL(cfhip_std_unpack_kernel<8>, grid, block, 0, stream, a); break;
		case 12: hipLaunchKernelGGL(cfhip_std_unpack_kernel<12>, grid, block, 0, stream, a); break;
		case 16: hipLaunchKernelGGL(cfhip_std_unpack_kernel<16>, grid, block, 0, stream, a); break;
		default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}
