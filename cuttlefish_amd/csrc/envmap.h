// envmap.h -- what cfhip_api.hip and envmap.hip share of the environment-map entries: panorama
// to cube faces, the GGX-prefiltered chain and the nine spherical-harmonic coefficients.  include/cuttlefish_hip.h has
// the definitions in full; tests/envmap_ref.py restates them in numpy.
//
//   faces        CubeFace order +X, -X, +Y, -Y, +Z, -Z; face size n, texel (x, y), y downward
//   s, t         s = 2 (x + 0.5) / n - 1, t = 2 (y + 0.5) / n - 1
//   d(f, s, t)   +X (1, -t, -s)  -X (-1, -t, s)  +Y (s, 1, t)  -Y (s, -1, -t)  +Z (s, -t, 1)  -Z (-s, -t, -1)
//   |d|^2        (dx^2 + dy^2) + dz^2;  n^ = d / sqrt(|d|^2), component by component
//   to a face    major axis X if |x| >= |y| and |x| >= |z|, else Y if |y| >= |z|, else Z; its sign picks the face;
//                (s, t) invert the table, divided by the major component's magnitude
//   fetch        px = (s + 1) 0.5 n - 0.5, x0 = floor(px), fx = px - x0, the same in y; a tap outside [0, n)^2 is
//                replaced by the nearest texel of the face its centre's direction selects; per channel
//                ((c00 (1 - fx) + c10 fx) (1 - fy)) + ((c01 (1 - fx) + c11 fx) fy)
//   sum64        p_j = sum of v_i, i = j mod 64, in increasing i from 0.0; p_j += p_{j xor 32}, 16, 8, 4, 2, 1; p_0
// All of it in IEEE double, in this order (the library is built with -ffp-contract=off).
#ifndef CFHIP_ENVMAP_H
#define CFHIP_ENVMAP_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cuttlefish_hip.h"

constexpr uint32_t CFENV_MAX_FACE = 8192;          // a face's side
constexpr uint32_t CFENV_MAX_PANORAMA = 32768;     // a panorama's width and height
constexpr uint32_t CFENV_MAX_LEVELS = 14;          // of an 8192^2 face
constexpr uint32_t CFENV_MIN_SAMPLES = 64;         // records of a sample table: a multiple of 64
constexpr uint32_t CFENV_MAX_SAMPLES = 4096;
constexpr uint32_t CFENV_WG_X = 64;                // a wavefront: 64 texels of a row, or the 64 sample classes of a texel
constexpr uint32_t CFENV_WG_Y = 4;                 // wavefronts of a workgroup
constexpr uint32_t CFENV_CHUNK = 1024;             // sample records staged in LDS at a time, 16 bytes each
constexpr uint32_t CFENV_SH_VALUES = 37;           // 9 coefficients x RGBA, then the sum of the solid angles
constexpr double CFENV_PI = 3.141592653589793;

// the real spherical-harmonic basis, in the order 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2: the constants the header
// quotes to six places (0.282095, 0.488603, 1.092548, 0.315392, 0.546274), in full
constexpr double CFENV_SH_C0 = 0.28209479177387814;
constexpr double CFENV_SH_C1 = 0.4886025119029199;
constexpr double CFENV_SH_C2 = 1.0925484305920792;
constexpr double CFENV_SH_C20 = 0.31539156525252005;
constexpr double CFENV_SH_C22 = 0.5462742152960396;

// What a launch of the prefilter sees.  src / dst: device tables of [6][levels] pointers, face-major; every level is
// tightly packed RGBA32F of size max(1, face_size >> level).
struct cfenv_prefilter_call {
	const void* const* src;
	void* const* dst;
	const cfhip_ggx_sample* table;     // device: `samples` records of destination level `level`
	uint32_t face_size, src_levels, dst_levels;
	uint32_t level, samples;
};

// one launch writes the six faces
extern "C" hipError_t cfhip_launch_equirect_to_cube(const void* src, int32_t src_type, uint32_t width, uint32_t height,
	unsigned long long src_pitch, void* const* faces, uint32_t face_size, uint32_t supersample, hipStream_t stream);
// one launch per destination level for the six faces: the lobe, or for samples == 0 the copy of source level `level`
extern "C" hipError_t cfhip_launch_cube_prefilter(const cfenv_prefilter_call* call, hipStream_t stream);
// rows: 6 * face_size records of CFENV_SH_VALUES doubles, the row partials
extern "C" hipError_t cfhip_launch_cube_sh9_rows(const void* const* faces, uint32_t face_size, double* rows, hipStream_t stream);
extern "C" hipError_t cfhip_launch_cube_sh9_final(const double* rows, uint32_t face_size, cfhip_sh9_result* result,
	hipStream_t stream);

// ---- the lobes beside GGX, the BRDF lookup table and the irradiance cube -----------------------
constexpr int CFENV_LOBE_GGX = 0, CFENV_LOBE_CHARLIE = 1, CFENV_LOBE_LAMBERT = 2;      // cfhip_lobe_sample_table's kind
constexpr uint32_t CFENV_MAX_LUT = 1024;           // a lookup table's width and height

// one launch: a wavefront per texel of the width x height table; table: device, `samples` records
extern "C" hipError_t cfhip_launch_brdf_lut(void* dst, uint32_t width, uint32_t height, const cfhip_hammersley_sample* table,
	uint32_t samples, uint32_t sheen, hipStream_t stream);
// one launch writes the six faces from the record cfhip_cube_sh9_device left on the device
extern "C" hipError_t cfhip_launch_cube_irradiance(const cfhip_sh9_result* sh, void* const* faces, uint32_t face_size,
	uint32_t over_pi, hipStream_t stream);

#endif
