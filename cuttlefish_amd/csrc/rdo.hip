// rdo.hip -- rate-distortion optimisation of BC1-5 / BC7 payloads (the definition of the
// pass is tests/rdo_ref.py).  The result is the payload with byte ranges of some blocks overwritten by the same
// byte range of one of the last L final blocks of the same segment of their block row, so that a deflate-class
// compressor finds matches.
//
//   * One wavefront per segment of CFRDO_SEG blocks; it walks the segment left to right, 64 blocks at a time:
//     lane j loads original block j of the run (one coalesced request), the steps take each block in turn through
//     v_readlane, lane j keeps final block j, and the run is stored in one request when it is done.  Every
//     original byte of a run is read before any of its bytes is written, so out == blocks works.
//   * Lanes are candidates: lane l owns candidates l and l + 64 (1 + L S of them; S splices per format).  Per step
//     a lane builds its candidate from the block's original bytes and the ring of the last L final blocks (LDS,
//     L x 16 bytes per wavefront), decodes it with decode4x4 and sums the squared error against the block's 16
//     source texels, which lanes 0..15 load (and quantise) once and the wave reads as uniform values.
//   * J = 16 SSE + round(16 lambda) R in integers, a wave argmin on (J, candidate), the winner's bytes go to the
//     ring and to lane j.
//   * Statistics: integer atomics per surface, one set per wavefront: their sums do not depend on the order.
//
// cfhip_rdo2d_kernel further down adds candidates from the block row above (tests/rdo2d_ref.py).
#include "decode_blocks.h"
#include "cf_device.h"
#include "cf_texel.h"
#include "rdo.h"

namespace {

constexpr int kL = CFRDO_LOOKBACK, kSeg = CFRDO_SEG;
static_assert(kSeg >= 64 && (kSeg & (kSeg - 1)) == 0, "a segment is a power of two of at least 64 blocks");
static_assert((kL & (kL - 1)) == 0, "the ring is indexed modulo L");
constexpr int kRows = CFRDO_TILE_ROWS, kUp = CFRDO_UP;
static_assert(kRows >= 1 && kUp >= 2 && kUp % 2 == 0 && kUp/2 <= 64, "dx = -UP/2 .. UP/2 - 1 stays within one run");

struct rdo_args {
	const cfrdo_entry* table;
	uint32_t n, total_seg;
	uint32_t lam16, cap, cmask;
	unsigned long long* stats;
};

// bytes [a, b) of a 16-byte block as a mask over its low (half 0) or high (half 1) eight bytes
constexpr uint64_t splice_mask(int a, int b, int half)
{
	uint64_t m = 0;
	for (int k = 0; k < 8; ++k)
		if (k + 8*half >= a && k + 8*half < b)
			m |= 0xFFull << (8*k);
	return m;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t lane)
{
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane);
	const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane);
	return ((uint64_t)hi << 32) | lo;
}

// the source texel as RGBA8: floats quantised as the encoders quantise them (cf_load_tile_rgba8)
__device__ __forceinline__ uint32_t source_texel(const uint8_t* row, uint32_t x, uint32_t pix)
{
	if (pix == 0u)
		return *reinterpret_cast<const uint32_t*>(row + (size_t)x*4u);
	const float4 f = pix == 1u ? load_rgbaf<1>(row, x) : load_rgbaf<2>(row, x);
	return cf_unorm8(f.x) | (cf_unorm8(f.y) << 8) | (cf_unorm8(f.z) << 16) | (cf_unorm8(f.w) << 24);
}

__device__ __forceinline__ void store_block(uint8_t* p, int bytes, bool vec, uint64_t lo, uint64_t hi)
{
	if (vec) {
		if (bytes == 16)
			*reinterpret_cast<uint4*>(p) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
		else
			*reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)lo, (uint32_t)(lo >> 32));
		return;
	}
	for (int i = 0; i < bytes; ++i)
		p[i] = (uint8_t)((i < 8 ? lo >> (8*i) : hi >> (8*(i - 8))) & 255u);
}

template <int ROW>
__global__ __launch_bounds__(64*CFRDO_WAVES) void cfhip_rdo_kernel(rdo_args t)
{
	constexpr cfrdo_row row = kCfrdoRows[ROW];
	constexpr int FMT = row.format, TYPE = row.type, BS = row.block_bytes, S = row.n;
	constexpr int NC = 1 + kL*S, SLOTS = (NC + 63)/64;
	constexpr int TB = texel_bytes<FMT, TYPE>();
	static_assert(SLOTS <= 2 && NC <= 256, "a lane owns at most two candidates; the key holds eight index bits");
	__shared__ uint64_t ring_all[CFRDO_WAVES][kL*2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t seg = cf_rfl(blockIdx.x*(uint32_t)CFRDO_WAVES + wave);
	if (seg >= t.total_seg)
		return;
	uint64_t* ring = ring_all[wave];
	// the surface of this segment: a wave-uniform binary search over seg_begin (cf_resolve's, cf_device.h)
	uint32_t lo_i = 0, hi_i = t.n - 1u;
	while (lo_i < hi_i) {
		const uint32_t mid = (lo_i + hi_i + 1u) >> 1;
		if (t.table[mid].seg_begin <= seg) lo_i = mid; else hi_i = mid - 1u;
	}
	const cfrdo_entry e = t.table[lo_i];
	const uint32_t local = seg - e.seg_begin;
	const uint32_t by = local/e.segx, x_begin = (local - by*e.segx)*(uint32_t)kSeg;
	const uint32_t nblk = e.bx - x_begin < (uint32_t)kSeg ? e.bx - x_begin : (uint32_t)kSeg;
	const bool vec = e.vec != 0;

	// this lane's candidates: the distance, the bytes it takes from there and its rate
	uint32_t cd[SLOTS], crate[SLOTS];
	uint64_t mlo[SLOTS], mhi[SLOTS];
	bool cvalid[SLOTS];
#pragma unroll
	for (int k = 0; k < SLOTS; ++k) {
		const uint32_t c = lane + 64u*k;
		cvalid[k] = c < (uint32_t)NC;
		cd[k] = 0; crate[k] = 8u*BS; mlo[k] = mhi[k] = 0;
		if (c >= 1u && cvalid[k]) {
			const uint32_t d = (c - 1u)/(uint32_t)S + 1u, s = (c - 1u) - (d - 1u)*(uint32_t)S;
			cd[k] = d;
#pragma unroll
			for (int q = 0; q < S; ++q)
				if (s == (uint32_t)q) {
					mlo[k] = splice_mask(row.a[q], row.b[q], 0);
					mhi[k] = splice_mask(row.a[q], row.b[q], 1);
					crate[k] = 8u*(uint32_t)(BS - (row.b[q] - row.a[q])) + 12u;
				}
			crate[k] += 2u*(31u - (uint32_t)__builtin_clz(d*(uint32_t)BS));
		}
	}
	// the compared channels as a byte mask over an RGBA8 word
	uint32_t bm = 0;
#pragma unroll
	for (int c = 0; c < 4; ++c)
		if (t.cmask & (1u << c))
			bm |= 255u << (8*c);

	uint32_t st_changed = 0, st_bits = 0;
	unsigned long long st_before = 0, st_after = 0;
	const uint32_t y0 = by*4u;
	const uint32_t ty = y0 + ((lane >> 2) & 3u);
	const bool ty_in = lane < 16u && ty < e.height;
	const uint8_t* prow = e.pixels + (unsigned long long)(ty_in ? ty : 0u)*e.pitch;

	for (uint32_t c0 = 0; c0 < nblk; c0 += 64u) {
		const uint32_t nb = nblk - c0 < 64u ? nblk - c0 : 64u;
		const size_t first = ((size_t)by*e.bx + x_begin + c0)*(size_t)BS;
		uint64_t olo = 0, ohi = 0;
		if (lane < nb)
			load_block(e.blocks + first + (size_t)lane*BS, BS, vec, olo, ohi);
		uint64_t flo = olo, fhi = ohi;
		// texel (lane & 3, lane >> 2) of the step's block, one step ahead of its use
		uint32_t px_next = 0;
		{
			const uint32_t tx = (x_begin + c0)*4u + (lane & 3u);
			if (ty_in && tx < e.width)
				px_next = source_texel(prow, tx, e.pix);
		}
		for (uint32_t i = 0; i < nb; ++i) {
			const uint32_t gi = c0 + i, x0 = (x_begin + gi)*4u;
			const uint32_t px = px_next;
			px_next = 0;
			if (i + 1u < nb) {
				const uint32_t tx = x0 + 4u + (lane & 3u);
				if (ty_in && tx < e.width)
					px_next = source_texel(prow, tx, e.pix);
			}
			const uint64_t cur_lo = readlane64(olo, i), cur_hi = readlane64(ohi, i);
			// the 16 source texels as uniform values, masked to the compared channels; texels outside the surface
			// compare nothing
			uint32_t src[16], tm[16];
#pragma unroll
			for (int k = 0; k < 16; ++k) {
				const bool in = x0 + (uint32_t)(k & 3) < e.width && y0 + (uint32_t)(k >> 2) < e.height;
				tm[k] = in ? bm : 0u;
				src[k] = (uint32_t)__builtin_amdgcn_readlane((int)px, k) & tm[k];
			}
			uint64_t klo[SLOTS], khi[SLOTS];
			uint32_t sse[SLOTS];
			bool ok[SLOTS];
#pragma unroll
			for (int k = 0; k < SLOTS; ++k) {
				ok[k] = cvalid[k] && cd[k] <= gi;
				klo[k] = cur_lo; khi[k] = cur_hi;
				sse[k] = 0;
				if (ok[k]) {
					const uint32_t slot = (gi - cd[k]) & (uint32_t)(kL - 1);
					const uint64_t rlo = ring[2u*slot], rhi = ring[2u*slot + 1u];
					klo[k] = (cur_lo & ~mlo[k]) | (rlo & mlo[k]);
					khi[k] = (cur_hi & ~mhi[k]) | (rhi & mhi[k]);
					// BC7's reserved mode is an error block: never a result (candidate 0 is the encoder's block)
					if (FMT == 36 && cd[k] != 0u && (klo[k] & 255u) == 0u)
						ok[k] = false;
				}
				if (ok[k]) {
					uint32_t w[4*TB];
					decode4x4<FMT, TYPE>(klo[k], khi[k], w);
					uint32_t acc = 0;
#pragma unroll
					for (int q = 0; q < 16; ++q) {
						uint32_t d;
						if constexpr (TB == 4) d = w[q];
						else if constexpr (TB == 1) d = (w[q >> 2] >> (8*(q & 3))) & 255u;
						else d = (w[q >> 1] >> (16*(q & 1))) & 0xFFFFu;
						d &= tm[q];
#pragma unroll
						for (int c = 0; c < (TB == 4 ? 4 : TB); ++c) {
							const int df = (int)((d >> (8*c)) & 255u) - (int)((src[q] >> (8*c)) & 255u);
							acc += (uint32_t)(df*df);
						}
					}
					sse[k] = acc;
				}
			}
			const uint32_t sse0 = (uint32_t)__builtin_amdgcn_readlane((int)sse[0], 0);
			const unsigned long long limit = (unsigned long long)sse0 + t.cap;
			unsigned long long key = ~0ull;
#pragma unroll
			for (int k = 0; k < SLOTS; ++k) {
				const uint32_t c = lane + 64u*k;
				if (ok[k] && (c == 0u || t.cap == 0xFFFFFFFFu || (unsigned long long)sse[k] <= limit)) {
					const unsigned long long j = 16ull*sse[k] + (unsigned long long)t.lam16*crate[k];
					const unsigned long long kk = (j << 8) | c;
					key = kk < key ? kk : key;
				}
			}
			const unsigned long long best = cf_wave_min_u64(key);
			const uint32_t wc = cf_rfl((uint32_t)best & 255u);
			const uint32_t wl = wc & 63u;
			uint64_t sel_lo = klo[0], sel_hi = khi[0];
			uint32_t sel_sse = sse[0], sel_rate = crate[0];
			if (SLOTS > 1 && wc >= 64u) {
				sel_lo = klo[SLOTS - 1]; sel_hi = khi[SLOTS - 1];
				sel_sse = sse[SLOTS - 1]; sel_rate = crate[SLOTS - 1];
			}
			const uint64_t win_lo = readlane64(sel_lo, wl), win_hi = readlane64(sel_hi, wl);
			st_before += sse0;
			st_after += (uint32_t)__builtin_amdgcn_readlane((int)sel_sse, (int)wl);
			st_bits += (uint32_t)__builtin_amdgcn_readlane((int)sel_rate, (int)wl);
			st_changed += (win_lo != cur_lo || win_hi != cur_hi) ? 1u : 0u;
			// the ring is read by every lane at the next step: keep the accesses of the two steps in order
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			__builtin_amdgcn_wave_barrier();
			if (lane == 0u) {
				ring[2u*(gi & (uint32_t)(kL - 1))] = win_lo;
				ring[2u*(gi & (uint32_t)(kL - 1)) + 1u] = win_hi;
			}
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			__builtin_amdgcn_wave_barrier();
			if (lane == i) {
				flo = win_lo;
				fhi = win_hi;
			}
		}
		if (lane < nb)
			store_block(e.out + first + (size_t)lane*BS, BS, vec, flo, fhi);
	}
	if (lane == 0u) {
		unsigned long long* s = t.stats + (size_t)lo_i*CFRDO_STATS;
		atomicAdd(s + 0, (unsigned long long)nblk);
		atomicAdd(s + 1, (unsigned long long)st_changed);
		atomicAdd(s + 2, st_before);
		atomicAdd(s + 3, st_after);
		atomicAdd(s + 4, (unsigned long long)nblk*8ull*BS);
		atomicAdd(s + 5, (unsigned long long)st_bits);
	}
}

// The 2-D pass (the definition is tests/rdo2d_ref.py): a block may also copy from UP positions of the block row above.
//
//   * One wavefront per tile of CFRDO_SEG x CFRDO_TILE_ROWS blocks (t.total_seg counts tiles here); it walks the
//     tile's rows top to bottom and each row as cfhip_rdo_kernel walks a segment.  Tiles are independent, and a row is
//     stored when it is done, after every original byte of it was read, so out == blocks works.
//   * Candidates 0 .. L S are cfhip_rdo_kernel's; candidate 1 + L S + u S + s takes splice s from the FINAL block at
//     position i + dx, dx = u - UP/2, of the row above in the same tile, at the rate of a match (bx - dx) BS bytes
//     back.  A lane owns up to three candidates.
//   * LDS per wavefront: the ring, and behind it the final blocks of the row above (SEG x 16 bytes).  A run of 64
//     blocks enters it when the next run of its row is done (or the row is), since that run still reads the row above
//     at the four positions to its left.
template <int ROW>
__global__ __launch_bounds__(64*CFRDO_WAVES) void cfhip_rdo2d_kernel(rdo_args t)
{
	constexpr cfrdo_row row = kCfrdoRows[ROW];
	constexpr int FMT = row.format, TYPE = row.type, BS = row.block_bytes, S = row.n;
	constexpr int NC = 1 + (kL + kUp)*S, SLOTS = (NC + 63)/64;
	constexpr int TB = texel_bytes<FMT, TYPE>();
	static_assert(SLOTS <= 3 && NC <= 256, "a lane owns at most three candidates; the key holds eight index bits");
	// BC7's decoder twice over is more than the compiler unrolls on request: its two slots stay a loop
	constexpr int UNROLL = FMT == 36 ? 1 : SLOTS;
	__shared__ uint64_t lds_all[CFRDO_WAVES][(kL + kSeg)*2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t tile = cf_rfl(blockIdx.x*(uint32_t)CFRDO_WAVES + wave);
	if (tile >= t.total_seg)
		return;
	uint64_t* ring = lds_all[wave];          // slots 0 .. L - 1: the ring; L + p: the final block at position p of the row above
	uint32_t lo_i = 0, hi_i = t.n - 1u;
	while (lo_i < hi_i) {
		const uint32_t mid = (lo_i + hi_i + 1u) >> 1;
		if (t.table[mid].tile_begin <= tile) lo_i = mid; else hi_i = mid - 1u;
	}
	const cfrdo_entry e = t.table[lo_i];
	const uint32_t local = tile - e.tile_begin;
	const uint32_t trow = local/e.segx, x_begin = (local - trow*e.segx)*(uint32_t)kSeg;
	const uint32_t nblk = e.bx - x_begin < (uint32_t)kSeg ? e.bx - x_begin : (uint32_t)kSeg;
	const uint32_t by0 = trow*(uint32_t)kRows;
	const uint32_t nrow = e.by - by0 < (uint32_t)kRows ? e.by - by0 : (uint32_t)kRows;
	const bool vec = e.vec != 0;

	// this lane's candidates: where it copies from (cd: the distance to the left; cup: from the row above at
	// position + cdx), the bytes it takes from there and its rate
	uint32_t cd[SLOTS], crate[SLOTS];
	int cdx[SLOTS];
	uint64_t mlo[SLOTS], mhi[SLOTS];
	bool cvalid[SLOTS], cup[SLOTS];
#pragma unroll
	for (int k = 0; k < SLOTS; ++k) {
		const uint32_t c = lane + 64u*k;
		cvalid[k] = c < (uint32_t)NC;
		cup[k] = false;
		cd[k] = 0; cdx[k] = 0; crate[k] = 8u*BS; mlo[k] = mhi[k] = 0;
		if (c >= 1u && cvalid[k]) {
			const uint32_t g = (c - 1u)/(uint32_t)S, s = (c - 1u) - g*(uint32_t)S;
#pragma unroll
			for (int q = 0; q < S; ++q)
				if (s == (uint32_t)q) {
					mlo[k] = splice_mask(row.a[q], row.b[q], 0);
					mhi[k] = splice_mask(row.a[q], row.b[q], 1);
					crate[k] = 8u*(uint32_t)(BS - (row.b[q] - row.a[q])) + 12u;
				}
			uint32_t back;                   // the match's distance in blocks
			if (g < (uint32_t)kL) {
				cd[k] = g + 1u;
				back = g + 1u;
			} else {
				cup[k] = true;
				cdx[k] = (int)(g - (uint32_t)kL) - kUp/2;
				// a position right of the surface's last block is never valid: any distance will do there
				back = (int)e.bx > cdx[k] ? (uint32_t)((int)e.bx - cdx[k]) : 1u;
			}
			crate[k] += 2u*(31u - (uint32_t)__builtin_clz(back*(uint32_t)BS));
		}
	}
	uint32_t bm = 0;
#pragma unroll
	for (int c = 0; c < 4; ++c)
		if (t.cmask & (1u << c))
			bm |= 255u << (8*c);

	uint32_t st_changed = 0, st_bits = 0;
	unsigned long long st_before = 0, st_after = 0;
	// the run of the current row that is not in the LDS row yet: lane j holds its final block j
	uint64_t plo = 0, phi = 0;
	uint32_t pc0 = 0, pnb = 0;
	auto publish = [&]() {
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		if (lane < pnb) {
			ring[2u*((uint32_t)kL + pc0 + lane)] = plo;
			ring[2u*((uint32_t)kL + pc0 + lane) + 1u] = phi;
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
	};

	for (uint32_t r = 0; r < nrow; ++r) {
		const uint32_t by = by0 + r, y0 = by*4u;
		const bool up_row = e.up != 0 && r != 0u;
		const uint32_t ty = y0 + ((lane >> 2) & 3u);
		const bool ty_in = lane < 16u && ty < e.height;
		const uint8_t* prow = e.pixels + (unsigned long long)(ty_in ? ty : 0u)*e.pitch;
		for (uint32_t c0 = 0; c0 < nblk; c0 += 64u) {
			const uint32_t nb = nblk - c0 < 64u ? nblk - c0 : 64u;
			const size_t first = ((size_t)by*e.bx + x_begin + c0)*(size_t)BS;
			uint64_t olo = 0, ohi = 0;
			if (lane < nb)
				load_block(e.blocks + first + (size_t)lane*BS, BS, vec, olo, ohi);
			uint64_t flo = olo, fhi = ohi;
			uint32_t px_next = 0;
			{
				const uint32_t tx = (x_begin + c0)*4u + (lane & 3u);
				if (ty_in && tx < e.width)
					px_next = source_texel(prow, tx, e.pix);
			}
			for (uint32_t i = 0; i < nb; ++i) {
				const uint32_t gi = c0 + i, x0 = (x_begin + gi)*4u;
				const uint32_t px = px_next;
				px_next = 0;
				if (i + 1u < nb) {
					const uint32_t tx = x0 + 4u + (lane & 3u);
					if (ty_in && tx < e.width)
						px_next = source_texel(prow, tx, e.pix);
				}
				const uint64_t cur_lo = readlane64(olo, i), cur_hi = readlane64(ohi, i);
				uint32_t src[16], tm[16];
#pragma unroll
				for (int k = 0; k < 16; ++k) {
					const bool in = x0 + (uint32_t)(k & 3) < e.width && y0 + (uint32_t)(k >> 2) < e.height;
					tm[k] = in ? bm : 0u;
					src[k] = (uint32_t)__builtin_amdgcn_readlane((int)px, k) & tm[k];
				}
				uint64_t klo[SLOTS], khi[SLOTS];
				uint32_t sse[SLOTS];
				bool ok[SLOTS];
#pragma unroll UNROLL
				for (int k = 0; k < SLOTS; ++k) {
					const int pos = (int)gi + cdx[k];
					ok[k] = cvalid[k] && (cup[k] ? up_row && pos >= 0 && pos < (int)nblk : cd[k] <= gi);
					klo[k] = cur_lo; khi[k] = cur_hi;
					sse[k] = 0;
					if (ok[k]) {
						const uint32_t slot = cup[k] ? (uint32_t)kL + (uint32_t)pos : (gi - cd[k]) & (uint32_t)(kL - 1);
						const uint64_t rlo = ring[2u*slot], rhi = ring[2u*slot + 1u];
						klo[k] = (cur_lo & ~mlo[k]) | (rlo & mlo[k]);
						khi[k] = (cur_hi & ~mhi[k]) | (rhi & mhi[k]);
						if (FMT == 36 && (cup[k] || cd[k] != 0u) && (klo[k] & 255u) == 0u)
							ok[k] = false;
					}
					if (ok[k]) {
						uint32_t w[4*TB];
						decode4x4<FMT, TYPE>(klo[k], khi[k], w);
						uint32_t acc = 0;
#pragma unroll
						for (int q = 0; q < 16; ++q) {
							uint32_t d;
							if constexpr (TB == 4) d = w[q];
							else if constexpr (TB == 1) d = (w[q >> 2] >> (8*(q & 3))) & 255u;
							else d = (w[q >> 1] >> (16*(q & 1))) & 0xFFFFu;
							d &= tm[q];
#pragma unroll
							for (int c = 0; c < (TB == 4 ? 4 : TB); ++c) {
								const int df = (int)((d >> (8*c)) & 255u) - (int)((src[q] >> (8*c)) & 255u);
								acc += (uint32_t)(df*df);
							}
						}
						sse[k] = acc;
					}
				}
				const uint32_t sse0 = (uint32_t)__builtin_amdgcn_readlane((int)sse[0], 0);
				const unsigned long long limit = (unsigned long long)sse0 + t.cap;
				unsigned long long key = ~0ull;
#pragma unroll
				for (int k = 0; k < SLOTS; ++k) {
					const uint32_t c = lane + 64u*k;
					if (ok[k] && (c == 0u || t.cap == 0xFFFFFFFFu || (unsigned long long)sse[k] <= limit)) {
						const unsigned long long j = 16ull*sse[k] + (unsigned long long)t.lam16*crate[k];
						const unsigned long long kk = (j << 8) | c;
						key = kk < key ? kk : key;
					}
				}
				const unsigned long long best = cf_wave_min_u64(key);
				const uint32_t wc = cf_rfl((uint32_t)best & 255u);
				const uint32_t wl = wc & 63u;
				uint64_t sel_lo = klo[0], sel_hi = khi[0];
				uint32_t sel_sse = sse[0], sel_rate = crate[0];
#pragma unroll
				for (int k = 1; k < SLOTS; ++k)
					if (wc >= 64u*k) {
						sel_lo = klo[k]; sel_hi = khi[k];
						sel_sse = sse[k]; sel_rate = crate[k];
					}
				const uint64_t win_lo = readlane64(sel_lo, wl), win_hi = readlane64(sel_hi, wl);
				st_before += sse0;
				st_after += (uint32_t)__builtin_amdgcn_readlane((int)sel_sse, (int)wl);
				st_bits += (uint32_t)__builtin_amdgcn_readlane((int)sel_rate, (int)wl);
				st_changed += (win_lo != cur_lo || win_hi != cur_hi) ? 1u : 0u;
				__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
				__builtin_amdgcn_wave_barrier();
				if (lane == 0u) {
					ring[2u*(gi & (uint32_t)(kL - 1))] = win_lo;
					ring[2u*(gi & (uint32_t)(kL - 1)) + 1u] = win_hi;
				}
				__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
				__builtin_amdgcn_wave_barrier();
				if (lane == i) {
					flo = win_lo;
					fhi = win_hi;
				}
			}
			if (lane < nb)
				store_block(e.out + first + (size_t)lane*BS, BS, vec, flo, fhi);
			// the run before this one has no reader of the row above left
			publish();
			plo = flo; phi = fhi;
			pc0 = c0; pnb = nb;
		}
		publish();
		pnb = 0;
	}
	if (lane == 0u) {
		unsigned long long* s = t.stats + (size_t)lo_i*CFRDO_STATS;
		const unsigned long long blocks = (unsigned long long)nblk*nrow;
		atomicAdd(s + 0, blocks);
		atomicAdd(s + 1, (unsigned long long)st_changed);
		atomicAdd(s + 2, st_before);
		atomicAdd(s + 3, st_after);
		atomicAdd(s + 4, blocks*8ull*BS);
		atomicAdd(s + 5, (unsigned long long)st_bits);
	}
}

template <int ROW>
hipError_t launch_row2d(const rdo_args& t, hipStream_t stream)
{
	const uint32_t wgs = (t.total_seg + CFRDO_WAVES - 1u)/CFRDO_WAVES;
	hipLaunchKernelGGL(cfhip_rdo2d_kernel<ROW>, dim3(wgs), dim3(64*CFRDO_WAVES), 0, stream, t);
	return hipGetLastError();
}

template <int ROW>
hipError_t launch_row(const rdo_args& t, hipStream_t stream)
{
	const uint32_t wgs = (t.total_seg + CFRDO_WAVES - 1u)/CFRDO_WAVES;
	hipLaunchKernelGGL(cfhip_rdo_kernel<ROW>, dim3(wgs), dim3(64*CFRDO_WAVES), 0, stream, t);
	return hipGetLastError();
}

} // namespace

extern "C" hipError_t cfhip_launch_rdo(int row, const cfrdo_entry* table, uint32_t n, uint32_t total_seg,
	uint32_t lam16, uint32_t cap, unsigned cmask, unsigned long long* stats, hipStream_t stream)
{
	static_assert(kCfrdoRowCount == 7, "one case per row below");
	rdo_args t;
	t.table = table; t.n = n; t.total_seg = total_seg;
	t.lam16 = lam16; t.cap = cap; t.cmask = cmask; t.stats = stats;
	if (!n || !total_seg)
		return hipSuccess;
	switch (row) {
		case 0: return launch_row<0>(t, stream);
		case 1: return launch_row<1>(t, stream);
		case 2: return launch_row<2>(t, stream);
		case 3: return launch_row<3>(t, stream);
		case 4: return launch_row<4>(t, stream);
		case 5: return launch_row<5>(t, stream);
		case 6: return launch_row<6>(t, stream);
		default: return hipErrorInvalidValue;
	}
}

extern "C" hipError_t cfhip_launch_rdo2d(int row, const cfrdo_entry* table, uint32_t n, uint32_t total_tile,
	uint32_t lam16, uint32_t cap, unsigned cmask, unsigned long long* stats, hipStream_t stream)
{
	static_assert(kCfrdoRowCount == 7, "one case per row below");
	rdo_args t;
	t.table = table; t.n = n; t.total_seg = total_tile;
	t.lam16 = lam16; t.cap = cap; t.cmask = cmask; t.stats = stats;
	if (!n || !total_tile)
		return hipSuccess;
	switch (row) {
		case 0: return launch_row2d<0>(t, stream);
		case 1: return launch_row2d<1>(t, stream);
		case 2: return launch_row2d<2>(t, stream);
		case 3: return launch_row2d<3>(t, stream);
		case 4: return launch_row2d<4>(t, stream);
		case 5: return launch_row2d<5>(t, stream);
		case 6: return launch_row2d<6>(t, stream);
		default: return hipErrorInvalidValue;
	}
}
