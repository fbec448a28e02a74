// decode_batch.h -- what the host side (cfhip_api.hip) and the kernels (decode.hip) of a batched decode share:
// the surface table of one launch and the launcher.  One launch decodes every surface of a call; its workgroups
// are numbered across the surfaces and each finds its surface by a binary search over wg_begin, as the
// encoders' cf_resolve does (cf_device.h).
#ifndef CF_DECODE_BATCH_H
#define CF_DECODE_BATCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CFDEC_WG 256          // threads (= blocks) of a workgroup of the lane-per-block kernels
#define CFDEC_ASTC_RUN 64     // blocks (and threads) of an ASTC workgroup: a run of one block row

// what a batched decode stores per texel
#define CFDEC_OUT_NATIVE (-1) // the layout cfhip_decoded_layout names
#define CFDEC_OUT_RGBA8 0     // R8 / RG8 expanded to RGBA8 (absent channels 0, 0, 255)
#define CFDEC_OUT_RGBA32F 1   // every layout normalised to four floats (absent channels 0, 0, 1)

struct cfdec_batch_entry {
	const uint8_t* blocks;
	uint8_t* out;
	unsigned long long out_pitch;
	uint32_t width, height, bx, by;
	uint32_t wg_begin;        // first workgroup of this surface
	uint32_t wgx;             // ASTC: workgroups per block row
	uint32_t out_vec;         // out and its pitch are 16-byte aligned
	uint32_t blk_vec;         // blocks is aligned to the block size
};

// format / type: a pair with a decoded layout; out: a CFDEC_OUT_* value that the pair supports (the caller
// maps a pixel type that equals the native layout to CFDEC_OUT_NATIVE).  table / errors: device pointers, n
// entries / n counters (errors may be null).  Grid: total_wg workgroups.
extern "C" hipError_t cfhip_launch_decode_batch(int format, int type, int out, const cfdec_batch_entry* table,
	uint32_t n, uint32_t total_wg, int bw, int bh, unsigned long long* errors, hipStream_t stream);

#endif
