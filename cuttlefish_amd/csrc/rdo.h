// rdo.h -- what the host side (cfhip_api.hip) and the kernel (rdo.hip) of the rate-distortion pass share: the
// constants of the algorithm, the splice table, the surface table of one launch and the launcher.
// The definition of the pass is tests/rdo_ref.py, that of its 2-D form tests/rdo2d_ref.py;
// every constant below has its twin there.
#ifndef CF_RDO_H
#define CF_RDO_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CFRDO_LOOKBACK 16     // L: a block may copy from the last L final blocks of its segment
#ifndef CFRDO_SEG
#define CFRDO_SEG 64          // blocks of a segment (a power of two >= 64); one wavefront walks one segment
#endif
#ifndef CFRDO_TILE_ROWS
#define CFRDO_TILE_ROWS 8     // block rows of a tile of the 2-D pass; one wavefront walks one tile (SEG x TILE_ROWS blocks)
#endif
#define CFRDO_UP 8            // positions of the row above a block may copy from: dx = u - UP/2, u = 0 .. UP - 1
#define CFRDO_WAVES 4         // wavefronts (segments, or tiles) of a workgroup
#define CFRDO_MAX_SPLICES 7

// One row per supported (format, type): the block size, the channels the format stores (bit c: channel c; BC1_RGB
// stores no alpha) and the splices as byte ranges [a, b).
struct cfrdo_row {
	int format, type, block_bytes;
	unsigned channels;
	int n;
	int a[CFRDO_MAX_SPLICES], b[CFRDO_MAX_SPLICES];
};

constexpr cfrdo_row kCfrdoRows[] = {
	{29, 0, 8, 7u, 3, {0, 0, 4}, {8, 4, 8}},                                              // BC1_RGB
	{30, 0, 8, 15u, 3, {0, 0, 4}, {8, 4, 8}},                                             // BC1_RGBA
	{31, 0, 16, 15u, 4, {0, 8, 8, 12}, {16, 16, 12, 16}},                                 // BC2: colour half only
	{32, 0, 16, 15u, 7, {0, 0, 8, 0, 2, 8, 12}, {16, 8, 16, 2, 8, 12, 16}},               // BC3
	{33, 0, 8, 1u, 3, {0, 0, 2}, {8, 2, 8}},                                              // BC4 UNorm
	{34, 0, 16, 3u, 7, {0, 0, 8, 0, 2, 8, 10}, {16, 8, 16, 2, 8, 10, 16}},                // BC5 UNorm
	{36, 0, 16, 15u, 3, {0, 8, 0}, {16, 16, 8}},                                          // BC7
};
constexpr int kCfrdoRowCount = (int)(sizeof(kCfrdoRows)/sizeof(kCfrdoRows[0]));

inline int cfrdo_find_row(int format, int type)
{
	for (int i = 0; i < kCfrdoRowCount; ++i)
		if (kCfrdoRows[i].format == format && kCfrdoRows[i].type == type)
			return i;
	return -1;
}

struct cfrdo_entry {
	const uint8_t* blocks;        // the payload as encoded
	uint8_t* out;                 // the result; may equal blocks
	const uint8_t* pixels;        // source texels, aligned to the texel size
	unsigned long long pitch;     // a multiple of the texel size
	uint32_t width, height, bx, by;
	uint32_t seg_begin;           // first segment (wavefront) of this surface
	uint32_t segx;                // segments per block row
	uint32_t pix;                 // cfhip_pixel_type of the source
	uint32_t vec;                 // blocks and out are aligned to the block size
	// the 2-D pass only
	uint32_t tile_begin;          // first tile (wavefront) of this surface; ceil(by / TILE_ROWS) x segx tiles, row-major
	uint32_t up;                  // the surface has up-candidates: the row above lies inside the compressor's window
};

// The six counters of a surface, in the order of cfhip_rdo_stats.
#define CFRDO_STATS 6

// row: index into kCfrdoRows.  table / stats: device pointers, n entries / n x CFRDO_STATS counters (zeroed by the
// caller).  lam16 = round(16 lambda); cap: max_sse_increase (0xFFFFFFFF: none); cmask: channels compared (already
// ANDed with the row's).  Grid: ceil(total_seg / CFRDO_WAVES) workgroups.
extern "C" hipError_t cfhip_launch_rdo(int row, const cfrdo_entry* table, uint32_t n, uint32_t total_seg,
	uint32_t lam16, uint32_t cap, unsigned cmask, unsigned long long* stats, hipStream_t stream);

// The 2-D pass (tests/rdo2d_ref.py): the same arguments with tiles for segments.  Grid: ceil(total_tile / CFRDO_WAVES).
extern "C" hipError_t cfhip_launch_rdo2d(int row, const cfrdo_entry* table, uint32_t n, uint32_t total_tile,
	uint32_t lam16, uint32_t cap, unsigned cmask, unsigned long long* stats, hipStream_t stream);

#endif
