// pvrtc_surf.h -- one row of the PVRTC1 encoder's surface table, shared by the kernels (pvrtc.hip) and the host
// entry points (cfhip_api.hip).  Every pass is one launch over all surfaces of a call; a work item finds its surface
// by a binary search over blk_off (per-block passes) or ph_off (refine phases).
#pragma once
#include <stdint.h>

struct cf_pvrtc_surf {
	const uint8_t* src;       // source row 0 (load pass)
	long long pitch;          // bytes between source rows, may be negative
	uint8_t* out;             // payload (pack pass)
	uint32_t pix;             // cfhip_pixel_type
	uint32_t w, h;            // source size (powers of two)
	uint32_t bx, by;          // block grid (>= 2 x 2)
	uint32_t blk_off;         // first block of this surface in the call's word array (texels: 16 * blk_off)
	uint32_t ph_off;          // first block of this surface in one refine phase's numbering
	uint32_t pad;
};
