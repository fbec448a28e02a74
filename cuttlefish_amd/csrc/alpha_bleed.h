// alpha_bleed.h -- what cfhip_api.hip and alpha_bleed.hip share of alpha bleeding: the call's
// geometry and the launchers.
#ifndef CFHIP_ALPHA_BLEED_H
#define CFHIP_ALPHA_BLEED_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cuttlefish_hip.h"

constexpr uint32_t CFAB_WG_X = 64;                 // a wavefront is 64 texels of one row
constexpr uint32_t CFAB_WG_Y = 4;                  // wavefronts of a workgroup, one row each
constexpr uint32_t CFAB_ROWS = 16;                 // rows a wavefront of the seed and fill passes walks per atomic
constexpr uint32_t CFAB_NONE = 0xFFFFFFFFu;        // the seed word of a texel without a seed
constexpr uint32_t CFAB_MAX_SIDE = 32768;          // a seed word holds x | y << 16, and d^2 stays below 2^31
constexpr uint64_t CFAB_MAX_TEXELS = 1ull << 31;   // of a call: 8 bytes of scratch per texel

// What every launch of a call sees.  The seed buffers hold width * height words per layer, tightly packed, layer after
// layer; a workgroup is 64 x 4 texels of one layer, 64 x 64 in the seed and fill passes (grid: x, y, layer).
struct cfab_call {
	void* const* images;               // device table: layers pointers
	unsigned long long pitch;
	uint32_t width, height;
	int32_t pixel_type;
	uint32_t flags;                    // CFHIP_BLEED_WRAP_*
};

extern "C" hipError_t cfhip_launch_alpha_bleed_seed(const cfab_call* call, uint32_t layers, float threshold, uint32_t* seeds,
	cfhip_bleed_result* results, hipStream_t stream);
// one step of the flood: step_x, step_y = the step, reduced modulo the size on a wrapped axis
extern "C" hipError_t cfhip_launch_alpha_bleed_step(const cfab_call* call, uint32_t layers, uint32_t step_x, uint32_t step_y,
	const uint32_t* seeds_in, uint32_t* seeds_out, hipStream_t stream);
// the last step fused with the fill and the counters; max_dist2 = max_distance^2, 0 for unlimited
extern "C" hipError_t cfhip_launch_alpha_bleed_fill(const cfab_call* call, uint32_t layers, uint32_t step_x, uint32_t step_y,
	uint32_t max_dist2, const uint32_t* seeds_in, cfhip_bleed_result* results, hipStream_t stream);

#endif
