// alpha_sdf.h -- what cfhip_api.hip and alpha_sdf.hip share of the signed distance field from alpha (DESIGN.md section
// 4.22): the call's geometry, the scratch layout and the launchers.
#ifndef CFHIP_ALPHA_SDF_H
#define CFHIP_ALPHA_SDF_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cuttlefish_hip.h"

constexpr uint32_t CFSD_WG_X = 64;                 // a wavefront is 64 texels of one row
constexpr uint32_t CFSD_WG_Y = 4;                  // wavefronts of a workgroup
constexpr uint32_t CFSD_ROWS = 16;                 // rows a wavefront of the classify pass walks per atomic
constexpr uint32_t CFSD_TILE = 64;                 // rows of a column-pass tile
constexpr uint32_t CFSD_MAX_SPREAD = 126;          // K = spread + 1 <= 127: a row distance and the class share a byte
constexpr uint32_t CFSD_MAX_SIDE = 32768;
constexpr uint64_t CFSD_MAX_TEXELS = 1ull << 31;   // source texels of a call
// the column pass stages its tile's rows and spread rows above and below them, 64 bytes each
constexpr uint32_t CFSD_LDS_ROWS = CFSD_TILE + 2u*CFSD_MAX_SPREAD;

// What every launch of a call sees.  Scratch, tightly packed, layer after layer: plane = one 64-bit word per 64 texels
// of a row, (width + 63) / 64 words per row (bit i of word j: texel 64 j + i is inside; 0 past the width); rows = one
// byte per texel, the row distance (1 ... K) | class << 7; e = 16 bits per texel, e | class << 15 (scale > 1 only).
struct cfsd_call {
	const void* const* src;            // device table: layers pointers
	void* const* dst;                  // device table: layers pointers
	unsigned long long src_pitch, dst_pitch;
	uint32_t width, height;            // of the source
	int32_t src_type, dst_type;
	uint32_t flags;                    // CFHIP_SDF_WRAP_*
	uint32_t spread, scale, channel_mask;
};

extern "C" hipError_t cfhip_launch_alpha_sdf_classify(const cfsd_call* call, uint32_t layers, float threshold, uint64_t* plane,
	cfhip_sdf_result* results, hipStream_t stream);
extern "C" hipError_t cfhip_launch_alpha_sdf_row(const cfsd_call* call, uint32_t layers, const uint64_t* plane, uint8_t* rows,
	hipStream_t stream);
// e: written when scale > 1; at scale 1 the pass stores the field itself and e is not touched
extern "C" hipError_t cfhip_launch_alpha_sdf_column(const cfsd_call* call, uint32_t layers, const uint8_t* rows, uint16_t* e,
	cfhip_sdf_result* results, hipStream_t stream);
// scale > 1 only
extern "C" hipError_t cfhip_launch_alpha_sdf_resolve(const cfsd_call* call, uint32_t layers, const uint16_t* e, hipStream_t stream);

#endif
