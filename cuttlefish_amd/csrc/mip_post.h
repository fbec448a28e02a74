// mip_post.h -- what cfhip_api.hip and mip_post.hip share of the mip post-pass: the surface
// table, the per-level search state and the launchers.
#ifndef CFHIP_MIP_POST_H
#define CFHIP_MIP_POST_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cuttlefish_hip.h"

constexpr uint32_t CFMP_WG = 256;                  // threads of a workgroup
constexpr uint32_t CFMP_PER_THREAD = 16;           // texels of a thread
constexpr uint32_t CFMP_CHUNK = CFMP_WG*CFMP_PER_THREAD;   // texels of a workgroup
constexpr uint32_t CFMP_SLOTS = 16;                // counters of a surface: one per candidate scale of a pass
constexpr uint32_t CFMP_SEARCH_PASSES = 6;         // 2^24 bit patterns between 1 and S_MAX (or S_MIN and 1), 16-way
constexpr uint32_t CFMP_BITS_ONE = 0x3F800000u, CFMP_BITS_MIN = 0x3E800000u, CFMP_BITS_MAX = 0x40800000u;   // 1, 1/4, 4
constexpr uint32_t CFMP_MAX_TEXELS = 1u << 30;     // of one surface: texel indices are 32-bit

// One surface of a call.  The generated levels come first in the table (in the order of the result records), the
// level-0 surfaces after them: the search passes launch workgroups for the first part only.
struct cfmp_surf {
	const uint8_t* pixels;
	unsigned long long pitch;
	unsigned long long plane_off;      // a level's alpha values in the compact plane (floats)
	uint32_t width, height;
	uint32_t n;                        // texels
	int32_t pixel_type;
	uint32_t wg_begin;                 // first workgroup of the surface in a launch
	uint32_t ref;                      // a level's level-0 surface (table index)
};

// The search of one level.  dir: +1 searching above 1, -1 below, 0 decided (scale_bits holds the scale).
// While searching: count(lo) = cnt_lo, count(hi) = cnt_hi and the answer's two candidates lie in [lo, hi].
struct cfmp_state {
	uint32_t lo, hi, cnt_lo, cnt_hi;
	uint32_t target, c1;
	int32_t dir;
	uint32_t scale_bits;
};

extern "C" hipError_t cfhip_launch_mip_post_gather(const cfmp_surf* tab, uint32_t nsurf, uint32_t nlev, uint32_t total_wg,
	float threshold, float s0, float s1, float s2, uint32_t ncand, uint32_t cstride, float* plane, uint32_t* counters,
	hipStream_t stream);
extern "C" hipError_t cfhip_launch_mip_post_count(const cfmp_surf* tab, uint32_t nlev, uint32_t total_wg, float threshold,
	const cfmp_state* state, const float* plane, uint32_t* counters, hipStream_t stream);
extern "C" hipError_t cfhip_launch_mip_post_decide(const cfmp_surf* tab, uint32_t nlev, int first, cfmp_state* state,
	uint32_t* counters, cfhip_mip_post_result* results, hipStream_t stream);
extern "C" hipError_t cfhip_launch_mip_post_apply(const cfmp_surf* tab, uint32_t nlev, uint32_t total_wg, uint32_t flags,
	const cfmp_state* state, hipStream_t stream);

#endif
