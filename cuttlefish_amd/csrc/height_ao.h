// height_ao.h -- what cfhip_api.hip and height_ao.hip share of ambient occlusion from height maps (DESIGN.md section
// 4.25): the definition, the tile, the table of a call and the launchers.
//
// The definition (include/cuttlefish_hip.h states the same; tests/height_ao_ref.py is its numpy twin):
//   height     h = the channel as a float (RGBA8 (float)(v / 255.0), half -> float, float as stored), not finite: 0;
//              H = (double)height * (double)h, exact
//   direction  d = q D/4 + i: base i of the first quadrant turned q times by (x, y) -> (-y, x); w_d = half the angle between
//              its neighbours over 2 pi; R_d = the largest k with k^2 (vx^2 + vy^2) <= R^2
//   gain       g(d, k) = 1.0 / ((double)k * sqrt((double)(vx^2 + vy^2))), with FALLOFF times
//              (1.0 - (double)(k^2 (vx^2 + vy^2)) / (double)((R + 1)^2))
//   horizon    m_d = max over k = 1 ... R_d of (H(p + k v_d) - H(p)) * g(d, k), a wrapped axis modulo its side, no sample
//              outside an unwrapped surface; t_d = fmax(0.0, m_d - (double)bias), no sample: 0
//   visibility vis_d = 1.0 / (1.0 + t_d*t_d), UNIFORM: 1.0 - t_d / sqrt(1.0 + t_d*t_d)
//   value      S = 0.0, S = S + w_d * vis_d for d = 0 ... D - 1; v = fmin(1.0, fmax(0.0, 1.0 - (double)strength * (1.0 - S)))
//
// Two launches per call, all layers in each (grid z): the plane kernel extracts h into a float32 plane of the context's
// scratch, the scan kernel stages a tile of it and a halo of R texels in LDS and walks every (d, k) from there.  A
// sample outside an unwrapped surface is staged as a NaN: fmax() drops it, and a direction without a sample keeps
// m_d = -inf, which gives t_d = 0.
#ifndef CFHIP_HEIGHT_AO_H
#define CFHIP_HEIGHT_AO_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cuttlefish_hip.h"

constexpr uint32_t CFHAO_TILE_W = 64;              // texels of a tile's row: one wavefront
constexpr uint32_t CFHAO_OWN_ROWS = 4;             // rows of a tile that a wavefront owns
constexpr uint32_t CFHAO_TILE_H = 16;              // rows of a tile at R <= 16: a workgroup of 256, four wavefronts
constexpr uint32_t CFHAO_TILE_H_WIDE = 64;         // ... and above: a workgroup of 1024, sixteen wavefronts
constexpr uint32_t CFHAO_WG = 256;                 // threads of the plane kernel's workgroup
constexpr uint32_t CFHAO_MAX_RADIUS = 64;
constexpr uint32_t CFHAO_MAX_DIRECTIONS = 32;
constexpr uint32_t CFHAO_MAX_SIDE = 32768;
constexpr uint32_t CFHAO_MAX_TEXELS = 1u << 30;    // of one surface
constexpr uint32_t CFHAO_MAX_LAYERS = 65535;
constexpr uint32_t CFHAO_MAX_GAINS = CFHAO_MAX_DIRECTIONS*CFHAO_MAX_RADIUS;
// The scan is compiled for three halo classes, so that a small radius keeps several workgroups on a CU.  Above R = 16
// the tile is 64 rows and the workgroup 1024 threads: the halo is staged once for four times the texels, and a CU that
// has room for one workgroup only still holds sixteen wavefronts.  A build's LDS is its tile with the class's halo on
// every side, one float a texel, and two words of the workgroup's record:
//   R <= 16:  96 x  48 words + 8 =  18440 bytes
//   R <= 32: 128 x 128 words + 8 =  65544 bytes
//   R <= 64: 192 x 192 words + 8 = 147464 bytes
constexpr uint32_t CFHAO_HALO_CLASSES[3] = {16, 32, 64};
constexpr uint32_t cfhao_tile_rows(uint32_t halo)
{
	return halo <= CFHAO_HALO_CLASSES[0] ? CFHAO_TILE_H : CFHAO_TILE_H_WIDE;
}
constexpr uint32_t cfhao_lds_bytes(uint32_t halo)
{
	return (CFHAO_TILE_W + 2u*halo)*(cfhao_tile_rows(halo) + 2u*halo)*4u + 8u;
}

// One direction of a call: its vector, its reach R_d, where its gains g(d, 1 ... R_d) start in the table, its weight
struct cfhao_dir {
	int32_t vx, vy;
	uint32_t reach, first;
	double weight;
};

// What the host makes once per call, in double, and uploads behind the pointer tables: uniform across the lanes
struct cfhao_table {
	cfhao_dir dir[CFHAO_MAX_DIRECTIONS];
	double gain[CFHAO_MAX_GAINS];
};

// What both launches of a call see.  Device tables: src and dst list `layers` pointers.
struct cfhao_call {
	const void* const* src;
	void* const* dst;
	const cfhao_table* table;
	unsigned long long src_pitch, dst_pitch;
	uint32_t width, height;
	int32_t src_type, dst_type;
	uint32_t flags, channel, directions, radius, channel_mask;
	float height_scale, strength, bias;
};

// plane: layers * height * width floats, tightly packed.  The plane launch also opens the records (occluded 0, darkest
// the bits of 1.0f), so the scan's atomics need no memset.
extern "C" hipError_t cfhip_launch_height_ao_plane(const cfhao_call* call, uint32_t layers, float* plane,
	cfhip_height_ao_result* results, hipStream_t stream);
extern "C" hipError_t cfhip_launch_height_ao_scan(const cfhao_call* call, uint32_t layers, const float* plane,
	cfhip_height_ao_result* results, hipStream_t stream);

#endif
