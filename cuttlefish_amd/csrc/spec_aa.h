// spec_aa.h -- what cfhip_api.hip and spec_aa.hip share of specular anti-aliasing: the
// definition, the call's geometry, the scratch layout and the launcher.
//
// The definition (include/cuttlefish_hip.h states the same; tests/spec_aa_ref.py is its numpy twin):
//   decode     RGBA8 (double)((float)(v / 255.0)); RGBA16F half -> double; RGBA32F as stored
//   normal     x = (double)c (SIGNED_NORMALS) or (double)c*2.0 - 1.0; RECONSTRUCT_Z: z = sqrt(fmax(0.0, 1.0 - (x*x + y*y)));
//              len = sqrt((x*x + y*y) + z*z); len not finite or not > 0: (0, 0, 1), else x/len; q = (int64)rint(n * 2^30)
//   roughness  r = the channel; r >= 0 false: 0; r > 1: 1; alpha = r*r (PERCEPTUAL) or r; qa = (int64)rint(alpha*alpha * 2^32)
//   footprint  level k's texel x: level-0 columns [x 2^k, (x + 1) 2^k), the level's last column to the width; rows alike.
//              Hierarchical: the children of x at level k are [2x, 2x + 2) of level k-1, the last x up to w_(k-1).
//   moments    Sx, Sy, Sz, Sa = the int64 sums of the quantised values over the footprint; N = its texels
//   finish     mx = (double)Sx / ((double)N * 2^30) ...; A2 = (double)Sa / ((double)N * 2^32); L2 = (mx*mx + my*my) + mz*mz;
//              L2 < 1 false: v = 0; else L2 > 0 false: v = max_variance; else L = sqrt(L2),
//              v = fmin((double)max_variance, (1.0 - L2) / (L * (3.0 - L2))); a2 = fmin(1.0, A2 + (double)variance_scale * v);
//              stored (float)sqrt(a2), PERCEPTUAL (float)sqrt(sqrt(a2))
// Integer sums do not depend on their order, so tile shape, launch split and arrival order cannot show in the result.
//
// A launch ("stage") takes the grid of level b = 5 * stage as its input -- the texels of level 0, or the moments the
// stage before left in the scratch -- and finishes levels b + 1 ... b + 5.  A workgroup owns one texel of level b + 5:
// a 32 x 32 tile of the input, the last tile of a row or column running to the edge (up to 63).  A surface of up to
// 32768 on a side has 15 generated levels: 3 launches at most, whatever the layers.
#ifndef CFHIP_SPEC_AA_H
#define CFHIP_SPEC_AA_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cuttlefish_hip.h"

constexpr uint32_t CFSA_WG = 256;                  // threads of a workgroup
constexpr uint32_t CFSA_STAGE_LEVELS = 5;          // levels a launch finishes
constexpr uint32_t CFSA_TILE = 1u << CFSA_STAGE_LEVELS;   // input texels per side of a tile; the last one up to 2*TILE - 1
constexpr uint32_t CFSA_MAX_STAGES = 3;            // launches of a call, at most
constexpr uint32_t CFSA_MAX_SIDE = 32768;
constexpr uint32_t CFSA_MAX_TEXELS = 1u << 30;     // of one surface: the int64 sums of Q30 / Q32 values fit
constexpr uint32_t CFSA_MAX_LAYERS = 65535;
// A tile's moments in LDS, four planes of int64: its levels b + 1 ... b + 5 hold at most 31^2, 15^2, 7^2, 3^2 and 1
constexpr uint32_t CFSA_LDS_ENTRIES = 31u*31u + 15u*15u + 7u*7u + 3u*3u + 1u;
// ... and the workgroup's share of five result records (clamped, saturated, max_added each, one word of padding)
constexpr uint32_t CFSA_LDS_BYTES = CFSA_LDS_ENTRIES*4u*8u + 16u*4u;

// the moments of one texel of level 5 or 10 in the scratch; N follows from the geometry
struct cfsa_moments {
	long long sx, sy, sz, sa;
};

// What every launch of a call sees.  Device tables: normals and rough0 list `layers` pointers, levels
// layers * (levels_count - 1).  Scratch, tightly packed, layer after layer: the moments of level 5, then of level 10.
struct cfsa_call {
	const void* const* normals;
	const void* const* rough0;         // NULL: base_roughness
	void* const* levels;
	unsigned long long normal_pitch, rough_pitch;
	uint32_t width, height;            // of level 0
	uint32_t levels_count;
	int32_t normal_type, rough_type;
	uint32_t flags, channel;
	float base_roughness, variance_scale, max_variance;
};

// stage 0 reads the texels; stage s > 0 reads `in`, the moments of level 5 s, and every stage that is not the last
// writes `out`, the moments of level 5 (s + 1)
extern "C" hipError_t cfhip_launch_spec_aa(const cfsa_call* call, uint32_t layers, uint32_t stage, const cfsa_moments* in,
	cfsa_moments* out, cfhip_spec_aa_result* results, hipStream_t stream);

#endif
