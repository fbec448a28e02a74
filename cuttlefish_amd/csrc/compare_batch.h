// compare_batch.h -- what the host side (cfhip_api.hip) and the kernels (compare.hip) of a batched compare share:
// the surface table of one call and the launchers.  Pass A, the SSIM pass and the final reduction are one launch
// each for every surface of the call; workgroups (Pass A), tiles (SSIM) and surfaces (final) are numbered across
// the table and a workgroup finds its entry by the binary search of the batched decode (decode_batch.h).
#ifndef CF_COMPARE_BATCH_H
#define CF_COMPARE_BATCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cuttlefish_hip.h"

struct cmp_batch_entry {
	const uint8_t* blocks;        // payload
	const uint8_t* ref;           // reference texels, aligned to the texel size
	unsigned long long ref_pitch; // a multiple of the texel size
	float* block_errors;          // error map of this surface, or null
	unsigned long long dec_off;   // SSIM: byte offset of the surface's decoded scratch (tight rows, native layout)
	uint32_t width, height, bx, by;
	uint32_t wg_begin;            // first Pass A workgroup = first Pass A partial (one partial per workgroup)
	uint32_t wgx;                 // ASTC: workgroups per block row
	uint32_t na;                  // Pass A workgroups (partials) of this surface
	uint32_t tile_begin;          // first SSIM tile = first SSIM partial
	uint32_t tiles_x, nb;         // SSIM tiles per tile row and in all; nb == 0: no valid window (or no SSIM pass)
	uint32_t windows;             // valid window centres
	uint32_t blk_vec;             // alignment flag: blocks is aligned to the block size
};

// Pass A of every surface: total_wg workgroups, partials receives total_wg x 16 doubles.
extern "C" hipError_t cfhip_launch_compare_batch(int format, int type, const cmp_batch_entry* table, uint32_t n,
	uint32_t total_wg, int bw, int bh, int ref_pix, unsigned cmask, double* partials, hipStream_t stream);

// The SSIM pass over total_tiles tiles; scratch + dec_off holds the decoded surfaces (cfhip_launch_decode_batch
// wrote them), partials receives total_tiles x 4 doubles.  taps / range as cfhip_launch_ssim.
extern "C" hipError_t cfhip_launch_ssim_batch(const cmp_batch_entry* table, uint32_t n, uint32_t total_tiles,
	const void* scratch, int layout, int ref_pix, unsigned cmask, const float* taps, double range, double* partials,
	hipStream_t stream);

// The final reduction, one workgroup per surface, into results[n] (device memory); pb null: no SSIM pass ran.
extern "C" hipError_t cfhip_launch_compare_batch_final(const cmp_batch_entry* table, uint32_t n, const double* pa,
	const double* pb, unsigned cmask, int hdr, cfhip_compare_result* results, hipStream_t stream);

#endif
