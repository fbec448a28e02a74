// cfhip_api.hip -- C-ABI shim (include/cuttlefish_hip.h) over the gfx950 kernels.
//
// Host-side counterpart of Converter::convert's per-surface loop
// (lib/src/Converter.cpp:521-589): for every surface upload (unless already
// resident), launch the format's kernel on the context stream, download the
// payload.  There is deliberately no CPU fallback here: without a HIP device
// cfhip_create() fails and the caller (HipConverter) keeps the reference path.
#include "cf_device.h"
#include "cf_texel.h"
#include "astc_tables.h"
#include "pvrtc_surf.h"
#include "compare_batch.h"
#include "decode_batch.h"
#include "rdo.h"
#include "lzsize.h"
#include "deflate.h"
#include "inflate.h"
#include "lz4.h"
#include "png.h"
#include "mip_post.h"
#include "alpha_bleed.h"
#include "alpha_sdf.h"
#include "spec_aa.h"
#include "height_ao.h"
#include "envmap.h"
#include "stage_log.h"
#include "../../include/cuttlefish_hip.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <new>
#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <sched.h>
#include <immintrin.h>

extern "C" hipError_t cfhip_launch_bc7(const cf_kparams* kp, int pixel_type, int unit_weights,
	hipStream_t stream);
extern "C" hipError_t cfhip_launch_astc(const cf_kparams* kp, int pixel_type, uint32_t nwaves, size_t lds_bytes, hipStream_t stream);
extern "C" void cfhip_astc_launch_shape(const cfastc::AstcBlobHeader* h, uint32_t quality, uint32_t hdr, uint32_t bx, uint32_t shape[4]);
extern "C" void cfhip_astc_plan(const cfastc::AstcBlobHeader* h, uint32_t quality, uint32_t hdr, uint32_t bx, uint32_t* nwaves, uint32_t* wcached, size_t* lds_bytes);
extern "C" hipError_t cfhip_launch_etc(const cf_kparams* kp, int format, int pixel_type, int snorm,
	hipStream_t stream);
extern "C" hipError_t cfhip_launch_bc6h(const cf_kparams* kp, int pixel_type, int is_signed,
	hipStream_t stream);
extern "C" hipError_t cfhip_launch_mip_resize(const void* src, int src_pixel_type, size_t pitch,
	uint32_t sw, uint32_t sh, void* dst, uint32_t dw, uint32_t dh, int filter, int srgb,
	hipStream_t stream);
extern "C" hipError_t cfhip_launch_mip_pass_layers(const void* src, int src_pixel_type, size_t pitch,
	uint32_t src_n, void* dst, uint32_t dst_w, uint32_t dst_h, int along_x, int filter, int to_linear,
	int to_srgb, uint32_t layers, const void* const* src_tab, void* const* dst_tab, size_t src_zstride,
	size_t dst_zstride, hipStream_t stream);
extern "C" hipError_t cfhip_launch_mip_fused_layers(const void* src, int src_pixel_type, size_t pitch, uint32_t sw,
	uint32_t sh, void* dst, uint32_t dw, uint32_t dh, int x_first, int filter, int srgb, uint32_t layers,
	const void* const* src_tab, void* const* dst_tab, size_t src_zstride, size_t dst_zstride, hipStream_t stream);
extern "C" hipError_t cfhip_launch_mip_pass(const void* src, int src_pixel_type, size_t pitch,
	uint32_t src_n, void* dst, uint32_t dst_w, uint32_t dst_h, int along_x, int filter, int to_linear,
	int to_srgb, hipStream_t stream);
extern "C" hipError_t cfhip_launch_image_ops(const void* src, int src_pixel_type, size_t pitch, uint32_t w,
	uint32_t h, const cfhip_image_ops* ops, void* dst, size_t dst_pitch, hipStream_t stream);
extern "C" hipError_t cfhip_launch_mip_depth(const void* prev, uint32_t n_prev, uint32_t texels, void* dst,
	uint32_t depth, int box, int srgb, hipStream_t stream);
extern "C" hipError_t cfhip_launch_std_pack(const cf_kparams* kp, int pixel_type, int bytes_per_pixel,
	hipStream_t stream);
extern "C" hipError_t cfhip_launch_std_unpack(int format, int type, int bytes_per_pixel, const void* pixels,
	uint32_t width, uint32_t height, void* out, size_t out_pitch, hipStream_t stream);
extern "C" uint64_t cfhip_std_compare_partials(uint32_t width, uint32_t height, uint64_t* ssim_partials);
extern "C" hipError_t cfhip_launch_std_compare(int format, int type, int bytes_per_pixel, const void* pixels,
	const void* ref, int ref_pix, size_t ref_pitch, uint32_t width, uint32_t height, unsigned cmask, int hdr,
	double* partials, hipStream_t stream);
extern "C" hipError_t cfhip_launch_decode(int format, int type, const void* blocks, int blk_vec, void* out,
	size_t out_pitch, const void* ref, size_t ref_pitch, int out_vec, uint32_t width, uint32_t height,
	uint32_t bx, uint32_t by, int bw, int bh, unsigned long long* acc, int sse, hipStream_t stream);
extern "C" uint64_t cfhip_compare_partials(int format, uint32_t width, uint32_t height, uint32_t bx, uint32_t by,
	uint64_t* ssim_partials);
extern "C" hipError_t cfhip_launch_compare(int format, int type, const void* blocks, int blk_vec, const void* ref,
	int ref_pix, size_t ref_pitch, uint32_t width, uint32_t height, uint32_t bx, uint32_t by, int bw, int bh,
	unsigned cmask, float* block_errors, double* partials, hipStream_t stream);
extern "C" hipError_t cfhip_launch_ssim(const void* dec, size_t dec_pitch, int layout, const void* ref, int ref_pix,
	size_t ref_pitch, uint32_t width, uint32_t height, unsigned cmask, const float* taps, double range,
	double* partials, hipStream_t stream);
extern "C" hipError_t cfhip_launch_compare_final(const double* pa, uint64_t na, const double* pb, uint64_t nb,
	unsigned cmask, int hdr, uint32_t windows, uint64_t texels, cfhip_compare_result* result, hipStream_t stream);
extern "C" hipError_t cfhip_pvrtc_launch(int pass, const cf_pvrtc_surf* tab, uint32_t n, uint32_t items,
	uint32_t* tex, uint32_t* words, uint8_t* mods, uint32_t wmask, int rgb, uint32_t ox, uint32_t oy, uint32_t flags,
	hipStream_t stream);
extern "C" hipError_t cfhip_pvrtc_launch_decode(const void* blocks, uint32_t w, uint32_t h, int rgb, void* out,
	size_t out_pitch, const void* ref, size_t ref_pitch, unsigned long long* sums, int sse, hipStream_t stream);
extern "C" hipError_t cfhip_launch_bc15(const cf_kparams* kp, int format, int pixel_type,
	int snorm, hipStream_t stream);

// Host worker pool of the pipelined host path: the threads live as long as the context (the reference
// creates and joins its worker threads per surface, Converter.cpp:557-583; per STRIP that would be tens of
// thread creations per call).  run(parts, fn) calls fn(part) for part = 0 .. parts-1, part 0 on the caller.
struct cf_host_pool {
	std::vector<std::thread> threads;
	std::mutex m;
	std::condition_variable wake, done;
	std::function<void(unsigned)> job;
	unsigned parts = 0, next = 0, pending = 0, generation = 0;
	bool stop = false;

	void worker()
	{
		unsigned seen = 0;
		std::unique_lock<std::mutex> lk(m);
		for (;;) {
			wake.wait(lk, [&] { return stop || generation != seen; });
			if (stop)
				return;
			seen = generation;
			while (next < parts) {
				const unsigned part = next++;
				lk.unlock();
				job(part);
				lk.lock();
				if (--pending == 0)
					done.notify_all();
			}
		}
	}
	void start(unsigned n)
	{
		for (unsigned i = 0; i < n; ++i)
			threads.emplace_back(&cf_host_pool::worker, this);
	}
	void run(unsigned nparts, const std::function<void(unsigned)>& fn)
	{
		if (nparts <= 1 || threads.empty()) {
			for (unsigned i = 0; i < nparts; ++i)
				fn(i);
			return;
		}
		std::unique_lock<std::mutex> lk(m);
		job = fn;
		parts = nparts;
		next = 1;                 // part 0 runs here
		pending = nparts;
		++generation;
		wake.notify_all();
		lk.unlock();
		fn(0);
		lk.lock();
		while (next < parts) {    // help with what is left
			const unsigned part = next++;
			lk.unlock();
			fn(part);
			lk.lock();
			--pending;
		}
		--pending;                // part 0
		done.wait(lk, [&] { return pending == 0; });
	}
	~cf_host_pool()
	{
		{
			std::lock_guard<std::mutex> lk(m);
			stop = true;
		}
		wake.notify_all();
		for (std::thread& t : threads)
			t.join();
	}
};

struct cfhip_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	void* d_src = nullptr;
	size_t src_cap = 0;
	void* d_out = nullptr;
	size_t out_cap = 0;
	void* d_batch = nullptr;          // cf_batch_entry[] of the current batched launch
	size_t batch_cap = 0;
	// pipelined host path: pinned strip slots, their events, the two copy streams beside `stream`, the pinned
	// payload buffer and the worker pool
	static constexpr int kPinSlots = 3;
	void* h_pin[kPinSlots] = {nullptr, nullptr, nullptr};
	size_t pin_cap = 0;
	hipEvent_t pin_free[kPinSlots] = {nullptr, nullptr, nullptr};   // slot's upload has left the host buffer
	hipEvent_t up_done[kPinSlots] = {nullptr, nullptr, nullptr};    // ... and arrived: the strip's kernel may start
	std::vector<hipEvent_t> strip_events;   // per strip: kernel finished / payload landed (grown on demand, reused)
	hipStream_t up_stream = nullptr, down_stream = nullptr;
	void* h_out = nullptr;            // pinned landing RING of the payload: kOutSlots strips (the caller's buffer is pageable)
	size_t h_out_cap = 0;
	static constexpr int kOutSlots = 4;
	cf_host_pool* pool = nullptr;
	// d_src / d_out / d_batch / d_mip3d are shared by every entry point, and calls on a caller's stream
	// return without synchronising: the last asynchronous user records this event and a call on
	// ANOTHER stream waits for it before touching the buffers.  Written by StagingLease alone.
	hipEvent_t staging_done = nullptr;
	hipEvent_t group_up = nullptr;    // grouped host path: the group's uploads have left the caller's buffers (release hook)
	hipStream_t staging_stream = nullptr;
	bool staging_busy = false;
	void* d_mip3d = nullptr;          // 3-D mip generation: the previous level's slices resized in x, y
	size_t mip3d_cap = 0;
	void* d_pvrtc = nullptr;          // PVRTC1 encoder state: surface table, texels, colour words, modulation bytes
	size_t pvrtc_cap = 0;
	void* d_lz = nullptr;             // deflate-size estimator: one slice's scratch (csrc/lzsize.h), grown on demand
	size_t lz_cap = 0;
	size_t lz_slice = 0;              // cfhip_lz_slice_bytes: 0 = CFLZ_SLICE_DEFAULT
	StageLog stages = {nullptr, 0, 0, 0, 0, 0};   // the last stream-codec call's event pairs by stage (csrc/stage_log.h)
	void* d_png = nullptr;            // cfhip_png_encode*: the filtered bytes, an unplaced zlib stream, the state (csrc/png.h)
	size_t png_cap = 0;
	void* d_rdo_keep = nullptr;       // cfhip_rdo_target: the pristine payloads every trial starts from
	size_t rdo_keep_cap = 0;
	std::map<int, void*> astc_tables; // per-format device tables (built on first use)
	std::map<int, cfastc::AstcBlobHeader> astc_hdr;   // their headers (sizes the launch's dynamic LDS)
	std::vector<hipEvent_t> events;   // start/stop pairs of the last call
	size_t events_used = 0;
	hipStream_t events_stream = nullptr;
	bool profiling = false;
	float last_ms = -1.0f;
	std::string last_kernel;
	std::string error;
	std::mutex lock;
};

namespace {

thread_local std::string g_error;

int fail(cfhip_ctx* ctx, int code, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	if (ctx)
		ctx->error = buf;
	g_error = buf;
	return code;
}

#define HIP_TRY(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
	return fail((ctx), CFHIP_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
// the same for a step that returns one of the library's own codes, its text already set
#define CF_TRY(expr) do { const int rc_ = (expr); if (rc_ != CFHIP_OK) return rc_; } while (0)

// ---- ASTC: footprints.  The per-footprint device table (partition lists, config lists, infill
// and quantisation tables) is built by csrc/astc_tables.h once per format and context.
bool astc_footprint(int format, int* bw, int* bh)
{
	static const unsigned char fp[14][2] = {{4, 4}, {5, 4}, {5, 5}, {6, 5}, {6, 6}, {8, 5}, {8, 6},
		{8, 8}, {10, 5}, {10, 6}, {10, 8}, {10, 10}, {12, 10}, {12, 12}};
	if (format < CFHIP_FORMAT_ASTC_4x4 || format > CFHIP_FORMAT_ASTC_12x12)
		return false;
	*bw = fp[format - CFHIP_FORMAT_ASTC_4x4][0];
	*bh = fp[format - CFHIP_FORMAT_ASTC_4x4][1];
	return true;
}

// ---- uncompressed ("standard") formats, Texture::Format 1..28 ----
// bytes per pixel for the (format, type) pairs createConverter accepts (Converter.cpp:38-337),
// 0 for the pairs it answers with nullptr.
bool is_std_format(int format)
{
	return format >= CFHIP_FORMAT_R4G4 && format <= CFHIP_FORMAT_E5B9G9R9_UFLOAT;
}

int std_pixel_bytes(int format, int type)
{
	const bool norm_or_int = type >= CFHIP_TYPE_UNORM && type <= CFHIP_TYPE_INT;
	switch (format) {
		case CFHIP_FORMAT_R4G4:
			return type == CFHIP_TYPE_UNORM ? 1 : 0;
		case CFHIP_FORMAT_R4G4B4A4: case CFHIP_FORMAT_B4G4R4A4: case CFHIP_FORMAT_A4R4G4B4:
		case CFHIP_FORMAT_R5G6B5: case CFHIP_FORMAT_B5G6R5: case CFHIP_FORMAT_R5G5B5A1:
		case CFHIP_FORMAT_B5G5R5A1: case CFHIP_FORMAT_A1R5G5B5:
			return type == CFHIP_TYPE_UNORM ? 2 : 0;
		case CFHIP_FORMAT_R8: return norm_or_int ? 1 : 0;
		case CFHIP_FORMAT_R8G8: return norm_or_int ? 2 : 0;
		case CFHIP_FORMAT_R8G8B8: return norm_or_int ? 3 : 0;
		case CFHIP_FORMAT_R8G8B8A8: return norm_or_int ? 4 : 0;
		case CFHIP_FORMAT_B8G8R8: return type == CFHIP_TYPE_UNORM ? 3 : 0;
		case CFHIP_FORMAT_B8G8R8A8: case CFHIP_FORMAT_A8B8G8R8:
			return type == CFHIP_TYPE_UNORM ? 4 : 0;
		case CFHIP_FORMAT_A2R10G10B10: case CFHIP_FORMAT_A2B10G10R10:
			return (type == CFHIP_TYPE_UNORM || type == CFHIP_TYPE_UINT) ? 4 : 0;
		case CFHIP_FORMAT_R16: case CFHIP_FORMAT_R16G16: case CFHIP_FORMAT_R16G16B16:
		case CFHIP_FORMAT_R16G16B16A16:
			return (norm_or_int || type == CFHIP_TYPE_FLOAT) ? 2*(format - CFHIP_FORMAT_R16 + 1) : 0;
		case CFHIP_FORMAT_R32: case CFHIP_FORMAT_R32G32: case CFHIP_FORMAT_R32G32B32:
		case CFHIP_FORMAT_R32G32B32A32:
			return (type == CFHIP_TYPE_UINT || type == CFHIP_TYPE_INT || type == CFHIP_TYPE_FLOAT)
				? 4*(format - CFHIP_FORMAT_R32 + 1) : 0;
		case CFHIP_FORMAT_B10G11R11_UFLOAT: case CFHIP_FORMAT_E5B9G9R9_UFLOAT:
			return type == CFHIP_TYPE_UFLOAT ? 4 : 0;
		default:
			return 0;
	}
}

int block_bytes(int format)
{
	switch (format) {
		case CFHIP_FORMAT_BC1_RGB:
		case CFHIP_FORMAT_BC1_RGBA:
		case CFHIP_FORMAT_BC4:
		case CFHIP_FORMAT_ETC1:
		case CFHIP_FORMAT_ETC2_R8G8B8:
		case CFHIP_FORMAT_ETC2_R8G8B8A1:
		case CFHIP_FORMAT_EAC_R11:
			return 8;
		case CFHIP_FORMAT_ETC2_R8G8B8A8:
		case CFHIP_FORMAT_EAC_R11G11:
			return 16;
		default:
			if (format >= CFHIP_FORMAT_ASTC_4x4 && format <= CFHIP_FORMAT_ASTC_12x12)
				return 16;
			return 0;
		case CFHIP_FORMAT_BC2:
		case CFHIP_FORMAT_BC3:
		case CFHIP_FORMAT_BC5:
		case CFHIP_FORMAT_BC6H:
		case CFHIP_FORMAT_BC7:
			return 16;
	}
}

void block_dims(int format, int* bw, int* bh)
{
	*bw = *bh = is_std_format(format) ? 1 : 4;
	astc_footprint(format, bw, bh);
}

// bytes of one output unit: a block, or a pixel of a standard format
int unit_bytes(int format, int type)
{
	return is_std_format(format) ? std_pixel_bytes(format, type) : block_bytes(format);
}

// createConverter's legality matrix, Converter.cpp:339-412
bool type_valid(int format, int type)
{
	if (is_std_format(format))
		return std_pixel_bytes(format, type) != 0;
	switch (format) {
		case CFHIP_FORMAT_BC1_RGB:
		case CFHIP_FORMAT_BC1_RGBA:
		case CFHIP_FORMAT_BC2:
		case CFHIP_FORMAT_BC3:
		case CFHIP_FORMAT_BC7:
			return type == CFHIP_TYPE_UNORM;
		case CFHIP_FORMAT_BC4:
		case CFHIP_FORMAT_BC5:
		case CFHIP_FORMAT_EAC_R11:       // Converter.cpp:424-430
		case CFHIP_FORMAT_EAC_R11G11:
			return type == CFHIP_TYPE_UNORM || type == CFHIP_TYPE_SNORM;
		case CFHIP_FORMAT_ETC1:          // Converter.cpp:414-422
		case CFHIP_FORMAT_ETC2_R8G8B8:
		case CFHIP_FORMAT_ETC2_R8G8B8A1:
		case CFHIP_FORMAT_ETC2_R8G8B8A8:
			return type == CFHIP_TYPE_UNORM;
		case CFHIP_FORMAT_BC6H:
			return type == CFHIP_TYPE_UFLOAT || type == CFHIP_TYPE_FLOAT;
		default:
			// ASTC: UNorm (LDR) and UFloat (HDR) are legal (Converter.cpp:431-488)
			if (format >= CFHIP_FORMAT_ASTC_4x4 && format <= CFHIP_FORMAT_ASTC_12x12)
				return type == CFHIP_TYPE_UNORM || type == CFHIP_TYPE_UFLOAT;
			return false;
	}
}

bool format_implemented(int format, int type)
{
	if (is_std_format(format))
		return true;
	// ASTC: UNorm = the LDR profile; UFloat = the HDR profiles (AstcConverter.cpp:150-162), encoded
	// with the HDR endpoint modes 11 / 14 / 15 in their direct sub-mode (csrc/astc_encode.hip)
	if (format >= CFHIP_FORMAT_ASTC_4x4 && format <= CFHIP_FORMAT_ASTC_12x12)
		return type == CFHIP_TYPE_UNORM || type == CFHIP_TYPE_UFLOAT;
	switch (format) {
		case CFHIP_FORMAT_BC1_RGB:
		case CFHIP_FORMAT_BC1_RGBA:
		case CFHIP_FORMAT_BC2:
		case CFHIP_FORMAT_BC3:
		case CFHIP_FORMAT_BC4:
		case CFHIP_FORMAT_BC5:
		case CFHIP_FORMAT_BC6H:
		case CFHIP_FORMAT_BC7:
		case CFHIP_FORMAT_ETC1:
		case CFHIP_FORMAT_ETC2_R8G8B8:
		case CFHIP_FORMAT_ETC2_R8G8B8A1:
		case CFHIP_FORMAT_ETC2_R8G8B8A8:
		case CFHIP_FORMAT_EAC_R11:
		case CFHIP_FORMAT_EAC_R11G11:
			return true;
		default:
			return false;
	}
}

size_t pixel_bytes(int pixel_type)
{
	return pixel_type >= CFHIP_PIXEL_RGBA8 && pixel_type <= CFHIP_PIXEL_RGBA16F ? cf_pixel_size(pixel_type) : 0;   // 0: no such type
}

int check_params(cfhip_ctx* ctx, const cfhip_params* p)
{
	if (!p)
		return fail(ctx, CFHIP_E_INVALID, "params is NULL");
	if (!unit_bytes(p->format, p->type) || !type_valid(p->format, p->type))
		return fail(ctx, CFHIP_E_UNSUPPORTED, "format %d / type %d is not a legal format "
			"(createConverter returns nullptr)", p->format, p->type);
	if (!format_implemented(p->format, p->type))
		return fail(ctx, CFHIP_E_UNSUPPORTED, "format %d / type %d has no gfx950 kernel yet",
			p->format, p->type);
	if (p->quality < 0 || p->quality > 4)
		return fail(ctx, CFHIP_E_INVALID, "quality %d out of range", p->quality);
	return CFHIP_OK;
}

void fill_kparams(cf_kparams& kp, const cfhip_params& p, const void* src, void* out,
	long long pitch, uint32_t w, uint32_t h)
{
	memset(&kp, 0, sizeof(kp));
	kp.src = static_cast<const uint8_t*>(src);
	kp.out = static_cast<uint8_t*>(out);
	kp.pitch = pitch;
	kp.width = w;
	kp.height = h;
	int fbw, fbh;
	block_dims(p.format, &fbw, &fbh);
	kp.bx = (w + (uint32_t)fbw - 1u)/(uint32_t)fbw;
	kp.by = (h + (uint32_t)fbh - 1u)/(uint32_t)fbh;
	kp.flags = is_std_format(p.format) ? (uint32_t)p.format : ((uint32_t)fbw | ((uint32_t)fbh << 8));
	kp.quality = (uint32_t)p.quality;
	kp.type = (uint32_t)p.type;
	// Colour mask (Texture::ColorMask; S3tcConverter.cpp:217-224 zeroes the weights):
	// a masked channel is made constant before the search so it cannot influence it.
	kp.keep_mask = 0;
	kp.set_mask = 0;
	for (int c = 0; c < 4; ++c)
		if (p.mask_rgba[c])
			kp.keep_mask |= 0xFFu << (8*c);
	if (!p.mask_rgba[3])
		kp.set_mask = 0xFF000000u;
	// channel weights: linear 1,1,1,1; sRGB at >= Normal asks for bc7enc's perceptual metric
	// (S3tcConverter.cpp:196-199): BC7 measures selector errors in (Y, Cr, Cb, A) with the axis
	// weights 16, 8, 2, 1 (kp.flags, one byte each; the colour mask zeroes the axis of its index
	// like the reference zeroes m_weights[c], :217-224) and uses the diagonal of that form,
	// 6,13,2,1, where a per-channel weight is needed; masked channels are constant so weight 1 is
	// harmless there
	static const uint32_t lin[4] = {1, 1, 1, 1}, perc[4] = {6, 13, 2, 1}, axes[4] = {16, 8, 2, 1};
	const bool perceptual = p.color_space == CFHIP_COLOR_SRGB && p.quality >= 2;
	const uint32_t* wsel = perceptual ? perc : lin;
	for (int c = 0; c < 4; ++c)
		kp.wt[c] = p.mask_rgba[c] ? wsel[c] : 1u;
	if (p.format == CFHIP_FORMAT_BC7) {
		kp.flags = perceptual ? 1u << 31 : 0u;     // bit 31: the perceptual kernel variant
		for (int c = 0; c < 4 && perceptual; ++c)
			kp.flags |= (p.mask_rgba[c] ? axes[c] : 0u) << (8*c);
	}
	if (p.format >= CFHIP_FORMAT_ETC1 && p.format <= CFHIP_FORMAT_EAC_R11G11) {
		// RGBX/RGBA metric for linear images, REC709 for sRGB (EtcConverter.cpp:60-88);
		// EtcConverter ignores the colour mask
		static const uint32_t elin[3] = {1, 1, 1}, erec[3] = {3, 10, 1};
		const uint32_t* w = p.color_space == CFHIP_COLOR_SRGB ? erec : elin;
		for (int c = 0; c < 3; ++c)
			kp.wt[c] = w[c];
	}
	if (p.format >= CFHIP_FORMAT_ASTC_4x4 && p.format <= CFHIP_FORMAT_ASTC_12x12) {
		// astcenc swizzle (AstcConverter.cpp:140-149): masked channel -> 0; alpha reads 1
		// when the texture has no alpha (Alpha::None), 0 when alpha is masked
		if (p.mask_rgba[3] && p.alpha == CFHIP_ALPHA_NONE) {
			kp.keep_mask &= 0x00FFFFFFu;
			kp.set_mask = 0xFF000000u;
		} else if (!p.mask_rgba[3])
			kp.set_mask = 0;
	}
	if (p.format == CFHIP_FORMAT_BC1_RGBA) {
		// punch-through blocks (squish path, S3tcConverter.cpp:294-330): Rec.709-like
		// integer weights for sRGB images, colour mask zeroes a channel's weight
		static const uint32_t plin[3] = {1, 1, 1}, pperc[3] = {3, 10, 1};
		const uint32_t* w = p.color_space == CFHIP_COLOR_SRGB ? pperc : plin;
		for (int c = 0; c < 3; ++c)
			kp.wt[c] = p.mask_rgba[c] ? w[c] : 0u;
	}
}

// the footprint's device tables, built on first use
int astc_prepare(cfhip_ctx* ctx, int format)
{
	void*& tab = ctx->astc_tables[format];
	if (tab)
		return CFHIP_OK;
	int fbw, fbh;
	astc_footprint(format, &fbw, &fbh);
	const std::vector<uint8_t> host = cfastc::build_blob(fbw, fbh);
	memcpy(&ctx->astc_hdr[format], host.data(), sizeof(cfastc::AstcBlobHeader));
	HIP_TRY(ctx, hipMalloc(&tab, host.size()));
	const hipError_t ce = hipMemcpy(tab, host.data(), host.size(), hipMemcpyHostToDevice);
	if (ce != hipSuccess) {
		// never leave a half-initialised table behind: the next call builds it again
		(void)hipFree(tab);
		tab = nullptr;
		return fail(ctx, CFHIP_E_DEVICE, "ASTC table upload: %s", hipGetErrorString(ce));
	}
	return CFHIP_OK;
}

// blocks of one block row a workgroup covers (the ASTC launch shape depends on the footprint)
int blocks_per_wg(cfhip_ctx* ctx, const cfhip_params& p, uint32_t quality, uint32_t bx, uint32_t* out)
{
	*out = CF_BLOCKS_PER_WG;
	if (p.format >= CFHIP_FORMAT_ASTC_4x4 && p.format <= CFHIP_FORMAT_ASTC_12x12) {
		const int rc = astc_prepare(ctx, p.format);
		if (rc != CFHIP_OK)
			return rc;
		uint32_t nwaves, wcached;
		size_t lds_bytes;
		cfhip_astc_plan(&ctx->astc_hdr[p.format], quality, p.type == CFHIP_TYPE_UFLOAT ? 1u : 0u, bx, &nwaves, &wcached, &lds_bytes);
		*out = nwaves*4u;
	}
	return CFHIP_OK;
}

int launch(cfhip_ctx* ctx, const cf_kparams& kp, const cfhip_params& p, int pixel_type,
	hipStream_t stream)
{
	hipError_t e;
	if (is_std_format(p.format)) {
		e = cfhip_launch_std_pack(&kp, pixel_type, std_pixel_bytes(p.format, p.type), stream);
		ctx->last_kernel = "cfhip_std_pack_kernel";
		if (e != hipSuccess)
			return fail(ctx, CFHIP_E_DEVICE, "kernel launch: %s", hipGetErrorString(e));
		return CFHIP_OK;
	}
	switch (p.format) {
		case CFHIP_FORMAT_BC7: {
			if (pixel_type != CFHIP_PIXEL_RGBA8 && pixel_type != CFHIP_PIXEL_RGBA32F)
				return fail(ctx, CFHIP_E_UNSUPPORTED, "BC7 takes RGBA8 or RGBA32F pixels");
			const int unit = !(kp.flags >> 31);
			e = cfhip_launch_bc7(&kp, pixel_type == CFHIP_PIXEL_RGBA32F ? 1 : 0, unit, stream);
			ctx->last_kernel = "cfhip_bc7_encode_kernel";
			break;
		}
		case CFHIP_FORMAT_ASTC_4x4: case CFHIP_FORMAT_ASTC_5x4: case CFHIP_FORMAT_ASTC_5x5:
		case CFHIP_FORMAT_ASTC_6x5: case CFHIP_FORMAT_ASTC_6x6: case CFHIP_FORMAT_ASTC_8x5:
		case CFHIP_FORMAT_ASTC_8x6: case CFHIP_FORMAT_ASTC_8x8: case CFHIP_FORMAT_ASTC_10x5:
		case CFHIP_FORMAT_ASTC_10x6: case CFHIP_FORMAT_ASTC_10x8: case CFHIP_FORMAT_ASTC_10x10:
		case CFHIP_FORMAT_ASTC_12x10: case CFHIP_FORMAT_ASTC_12x12: {
			if (pixel_type != CFHIP_PIXEL_RGBA8 && pixel_type != CFHIP_PIXEL_RGBA32F && pixel_type != CFHIP_PIXEL_RGBA16F)
				return fail(ctx, CFHIP_E_UNSUPPORTED, "ASTC takes RGBA8, RGBA16F or RGBA32F pixels");
			const int trc = astc_prepare(ctx, p.format);
			if (trc != CFHIP_OK)
				return trc;
			uint32_t nwaves, wcached;
			size_t lds_bytes;
			const uint32_t hdr = p.type == CFHIP_TYPE_UFLOAT ? 1u : 0u;
			// HDR profile (AstcConverter.cpp:150-162): HDR_RGB_LDR_A for Alpha::None / PreMultiplied, HDR otherwise
			const uint32_t hdr_alpha = hdr && !(p.alpha == CFHIP_ALPHA_NONE || p.alpha == CFHIP_ALPHA_PREMULTIPLIED) ? 1u : 0u;
			cfhip_astc_plan(&ctx->astc_hdr[p.format], kp.quality, hdr, kp.bx, &nwaves, &wcached, &lds_bytes);
			cf_kparams k2 = kp;
			k2.aux = ctx->astc_tables[p.format];
			k2.flags |= (wcached << 18) | (hdr << 19) | (hdr_alpha << 20);
			// ASTCENC_FLG_USE_ALPHA_WEIGHT for Alpha::Standard / PreMultiplied, USE_PERCEPTUAL for sRGB
			// images (AstcConverter.cpp:163-172)
			k2.flags |= ((p.alpha == CFHIP_ALPHA_STANDARD || p.alpha == CFHIP_ALPHA_PREMULTIPLIED) ? 1u << 16 : 0u) |
				(p.color_space == CFHIP_COLOR_SRGB ? 1u << 17 : 0u);
			// a half-float source runs the float kernel with bit 21 set: its loader reads 8 bytes per texel
			k2.flags |= pixel_type == CFHIP_PIXEL_RGBA16F ? 1u << 21 : 0u;
			e = cfhip_launch_astc(&k2, pixel_type == CFHIP_PIXEL_RGBA8 ? 0 : 1, nwaves, lds_bytes, stream);
			ctx->last_kernel = "cfhip_astc_encode_kernel";
			break;
		}
		case CFHIP_FORMAT_ETC1:
		case CFHIP_FORMAT_ETC2_R8G8B8:
		case CFHIP_FORMAT_ETC2_R8G8B8A1:
		case CFHIP_FORMAT_ETC2_R8G8B8A8:
		case CFHIP_FORMAT_EAC_R11:
		case CFHIP_FORMAT_EAC_R11G11:
			if (pixel_type != CFHIP_PIXEL_RGBA8 && pixel_type != CFHIP_PIXEL_RGBA32F)
				return fail(ctx, CFHIP_E_UNSUPPORTED, "ETC/EAC take RGBA8 or RGBA32F pixels");
			e = cfhip_launch_etc(&kp, p.format, pixel_type == CFHIP_PIXEL_RGBA32F ? 1 : 0,
				p.type == CFHIP_TYPE_SNORM ? 1 : 0, stream);
			ctx->last_kernel = "cfhip_etc_encode_kernel";
			break;
		case CFHIP_FORMAT_BC6H:
			e = cfhip_launch_bc6h(&kp, pixel_type, p.type == CFHIP_TYPE_FLOAT ? 1 : 0, stream);
			ctx->last_kernel = "cfhip_bc6h_encode_kernel";
			break;
		case CFHIP_FORMAT_BC1_RGB:
		case CFHIP_FORMAT_BC1_RGBA:
		case CFHIP_FORMAT_BC2:
		case CFHIP_FORMAT_BC3:
		case CFHIP_FORMAT_BC4:
		case CFHIP_FORMAT_BC5:
			if (pixel_type != CFHIP_PIXEL_RGBA8 && pixel_type != CFHIP_PIXEL_RGBA32F)
				return fail(ctx, CFHIP_E_UNSUPPORTED, "BC1-5 take RGBA8 or RGBA32F pixels");
			e = cfhip_launch_bc15(&kp, p.format, pixel_type == CFHIP_PIXEL_RGBA32F ? 1 : 0,
				p.type == CFHIP_TYPE_SNORM ? 1 : 0, stream);
			ctx->last_kernel = "cfhip_bc15_encode_kernel";
			break;
		default:
			return fail(ctx, CFHIP_E_UNSUPPORTED, "format %d has no gfx950 kernel yet", p.format);
	}
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "kernel launch: %s", hipGetErrorString(e));
	return CFHIP_OK;
}

int next_event_pair(cfhip_ctx* ctx, hipEvent_t* a, hipEvent_t* b)
{
	if (ctx->events_used + 2 > ctx->events.size()) {
		for (int i = 0; i < 2; ++i) {
			hipEvent_t ev;
			HIP_TRY(ctx, hipEventCreate(&ev));
			ctx->events.push_back(ev);
		}
	}
	*a = ctx->events[ctx->events_used];
	*b = ctx->events[ctx->events_used + 1];
	ctx->events_used += 2;
	return CFHIP_OK;
}

// One timed span on the stream (cfhip_last_kernel_ms / profiling): an event pair around what `launch` enqueues, one
// kernel or several; it returns the first hipError_t that is no success.  `what` names the family in the error text.
template <class Launch>
int timed(cfhip_ctx* ctx, hipStream_t stream, const char* what, Launch&& launch)
{
	hipEvent_t a, b;
	const int rc = next_event_pair(ctx, &a, &b);
	if (rc != CFHIP_OK)
		return rc;
	HIP_TRY(ctx, hipEventRecord(a, stream));
	const hipError_t e = launch();
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "%s launch: %s", what, hipGetErrorString(e));
	HIP_TRY(ctx, hipEventRecord(b, stream));
	return CFHIP_OK;
}

// The encoders' form of it: launch() picks the kernel, names it in last_kernel and formats its own errors (an
// unsupported pixel type among them), so it returns an int and stays apart from timed().
int timed_launch(cfhip_ctx* ctx, const cf_kparams& kp, const cfhip_params& p, int pixel_type,
	hipStream_t stream)
{
	hipEvent_t a, b;
	int rc = next_event_pair(ctx, &a, &b);
	if (rc != CFHIP_OK)
		return rc;
	HIP_TRY(ctx, hipEventRecord(a, stream));
	rc = launch(ctx, kp, p, pixel_type, stream);
	if (rc != CFHIP_OK)
		return rc;
	HIP_TRY(ctx, hipEventRecord(b, stream));
	return CFHIP_OK;
}

int reserve(cfhip_ctx* ctx, void** buf, size_t* cap, size_t need)
{
	if (need <= *cap)
		return CFHIP_OK;
	if (*buf) {
		HIP_TRY(ctx, hipFree(*buf));
		*buf = nullptr;
		*cap = 0;
	}
	HIP_TRY(ctx, hipMalloc(buf, need));
	*cap = need;
	return CFHIP_OK;
}

// The one owner of the staging buffers (d_src, d_out, d_batch, d_mip3d, and the estimator's d_lz and the target
// search's d_rdo_keep, the PNG writer's d_png) for one call on one stream; the only code
// that writes staging_busy / staging_stream / staging_done.  Declared after the context's lock guard (inside the body
// that guarded() runs), so that it ends before the lock is released.
//  * acquire(): before the first touch of a buffer; the first call makes the stream wait for the last asynchronous
//    user when that was another stream (same-stream reuse is ordered anyway).  The entry point, its host wrapper or
//    the target search acquires; the stream codecs' *_run routines never do.
//  * done(synchronous): the only success exit.  An asynchronous call that acquired records staging_done and becomes
//    the last user; a synchronous one drains its stream, after which the buffers are idle if it acquired (its stream
//    waited for the previous user) or was the last user itself.
//  * any other exit (an error return, an exception unwinding to guarded()): a call that acquired drains its stream
//    and the host pipeline's copy streams, and the buffers are idle once that succeeded; a call that never acquired
//    leaves their state as it found it -- another stream's work may still be in flight on them.
struct StagingLease {
	cfhip_ctx* const ctx;
	const hipStream_t stream;
	bool acquired = false, finished = false;

	StagingLease(cfhip_ctx* c, hipStream_t s) : ctx(c), stream(s) {}
	StagingLease(const StagingLease&) = delete;
	StagingLease& operator=(const StagingLease&) = delete;

	int acquire()
	{
		if (!acquired && ctx->staging_busy && ctx->staging_stream != stream)
			HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->staging_done, 0));
		acquired = true;
		return CFHIP_OK;
	}

	int done(bool synchronous)
	{
		if (synchronous) {
			HIP_TRY(ctx, hipStreamSynchronize(stream));
			if (acquired || ctx->staging_stream == stream)
				ctx->staging_busy = false;
		} else if (acquired) {
			if (!ctx->staging_done)
				HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->staging_done, hipEventDisableTiming));
			HIP_TRY(ctx, hipEventRecord(ctx->staging_done, stream));
			ctx->staging_stream = stream;
			ctx->staging_busy = true;
		}
		finished = true;
		return CFHIP_OK;
	}

	~StagingLease()
	{
		if (finished)
			return;
		if (acquired) {
			// (the copy streams are idle unless the host pipeline ran: draining them is free otherwise)
			bool drained = hipStreamSynchronize(stream) == hipSuccess;
			if (ctx->up_stream) drained = hipStreamSynchronize(ctx->up_stream) == hipSuccess && drained;
			if (ctx->down_stream) drained = hipStreamSynchronize(ctx->down_stream) == hipSuccess && drained;
			if (drained)
				ctx->staging_busy = false;
		}
		// the error's text is in ctx->error; a runtime error left behind would fail the next launch's check
		(void)hipGetLastError();
	}
};

// ---- what every entry point that works on a context shares ---------------------------------------------------------
// No exception across the C boundary: std::bad_alloc / std::system_error from the vectors and threads of a body become
// CFHIP_E_DEVICE with the text in cfhip_last_error.  On its own only where no single context's lock fits: the planning
// of cfhip_encode_multi_ex, which runs guarded calls on every context.
template <class Body>
int no_throw(cfhip_ctx* ctx, const char* what, Body&& body)
{
	try {
		return body();
	} catch (const std::exception& e) {
		return fail(ctx, CFHIP_E_DEVICE, "%s: %s", what, e.what());
	} catch (...) {
		return fail(ctx, CFHIP_E_DEVICE, "%s: unknown exception", what);
	}
}

// An entry point's frame: the context's lock while the body runs (none for a NULL context: the checks and the
// empty-input answers need none), its error text cleared, and no exception out of it.  The body makes the checks in the
// entry point's own order -- the NULL-context check first or after the argument checks -- and declares its StagingLease
// itself, so the lease ends, also while an exception unwinds, before the lock is released.
template <class Body>
int guarded(cfhip_ctx* ctx, const char* what, Body&& body)
{
	std::unique_lock<std::mutex> guard;
	if (ctx) {
		guard = std::unique_lock<std::mutex>(ctx->lock);
		ctx->error.clear();
	}
	return no_throw(ctx, what, body);
}

// the stream a call works on: the caller's, or the context's own
hipStream_t call_stream(cfhip_ctx* ctx, void* stream_)
{
	return stream_ ? static_cast<hipStream_t>(stream_) : ctx->stream;
}

// The event bookkeeping of a call that starts: its pairs are counted from here (all pairs, while profiling), and the
// stage log of the call before it is closed.  kernel: what the call leaves in last_kernel; NULL where the call names it
// only when it launches (the encoders' launch()), so that a call that fails before that leaves the name as it found it.
void begin_call(cfhip_ctx* ctx, hipStream_t stream, const char* kernel)
{
	if (!ctx->profiling)
		ctx->events_used = 0;
	ctx->events_stream = stream;
	ctx->last_ms = -1.0f;
	if (kernel)
		ctx->last_kernel = kernel;
	ctx->stages.owner = nullptr;
}

// ---- the image passes on device surfaces (mip post-pass, alpha bleeding, distance field, specular AA, environment
// maps): one frame for what follows their argument checks, one vocabulary for the checks themselves ------------------
// The frame, inside the body that guarded() runs: the NULL context reported last, the device, the lease on the call's
// stream, the event reset with the name the call leaves in last_kernel, the two staging buffers at the sizes the pass
// takes (0: not taken), then body(stream) -- the uploads and launches -- and the lease's success exit.  Any failure
// returns with the lease unfinished, which drains what was enqueued.
template <class Body>
int device_pass(cfhip_ctx* ctx, void* stream_, const char* kernel, size_t batch_bytes, size_t src_bytes, Body&& body)
{
	if (!ctx)
		return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	StagingLease lease(ctx, call_stream(ctx, stream_));
	begin_call(ctx, lease.stream, kernel);
	CF_TRY(lease.acquire());
	CF_TRY(reserve(ctx, &ctx->d_batch, &ctx->batch_cap, batch_bytes));
	CF_TRY(reserve(ctx, &ctx->d_src, &ctx->src_cap, src_bytes));
	CF_TRY(body(lease.stream));
	return lease.done(!stream_);
}

// Host tables of pointers, one after the other into d_batch: slots[i] is where tabs[i] went.  A table of no entries
// takes no room and is not read.  Pageable sources: the runtime stages each copy before returning.
struct PtrTable {
	const void* const* host;
	size_t count;
};

template <size_t N>
int upload_tables(cfhip_ctx* ctx, hipStream_t stream, const PtrTable (&tabs)[N], void** (&slots)[N])
{
	void** at = static_cast<void**>(ctx->d_batch);
	for (size_t i = 0; i < N; at += tabs[i++].count) {
		slots[i] = at;
		if (tabs[i].count)
			HIP_TRY(ctx, hipMemcpyAsync(at, tabs[i].host, tabs[i].count*sizeof(void*), hipMemcpyHostToDevice, stream));
	}
	return CFHIP_OK;
}

// A pass's launches, every one a timed span of its own; after the first failure the rest are skipped and rc keeps it.
struct LaunchChain {
	cfhip_ctx* ctx;
	hipStream_t stream;
	const char* what;
	int rc = CFHIP_OK;

	LaunchChain(cfhip_ctx* c, hipStream_t s, const char* w) : ctx(c), stream(s), what(w) {}

	template <class Launch>
	void operator()(Launch&& launch)
	{
		if (rc == CFHIP_OK)
			rc = timed(ctx, stream, what, launch);
	}
};

// The levels of a full chain: floor(log2(max(w, h))) + 1 (maxMipmapLevels, Texture.cpp)
uint32_t chain_levels(uint32_t width, uint32_t height)
{
	uint32_t levels = 1;
	for (uint32_t d = std::max(width, height); d > 1; d >>= 1)
		++levels;
	return levels;
}

uint32_t cube_levels(uint32_t face_size)
{
	return chain_levels(face_size, face_size);
}

// The checks' vocabulary: `what` names the pass, `name` the argument as the header spells it.  Every pass calls them in
// its own order, the per-element ones from its own loop over the layers: which fault of several is reported is part of
// the ABI.
int check_given(cfhip_ctx* ctx, const char* what, const char* name, const void* p)
{
	return p ? CFHIP_OK : fail(ctx, CFHIP_E_INVALID, "%s: %s is NULL", what, name);
}

int check_layers(cfhip_ctx* ctx, const char* what, uint32_t layers)
{
	if (!layers || layers > 65535u)
		return fail(ctx, CFHIP_E_INVALID, "%s: layers is %u (1 to 65535 per call)", what, layers);
	return CFHIP_OK;
}

int check_sides(cfhip_ctx* ctx, const char* what, uint32_t width, uint32_t height, uint32_t max_side)
{
	if (!width || !height || width > max_side || height > max_side)
		return fail(ctx, CFHIP_E_INVALID, "%s: width and height are 1 to %u each, not %ux%u", what, max_side, width, height);
	return CFHIP_OK;
}

// *bytes: a texel of the pixel type
int check_pixel_type(cfhip_ctx* ctx, const char* what, const char* name, int pixel_type, size_t* bytes)
{
	*bytes = pixel_bytes(pixel_type);
	return *bytes ? CFHIP_OK : fail(ctx, CFHIP_E_INVALID, "%s: %s %d", what, name, pixel_type);
}

int check_row_pitch(cfhip_ctx* ctx, const char* what, const char* name, size_t pitch, size_t row)
{
	return pitch >= row ? CFHIP_OK : fail(ctx, CFHIP_E_INVALID, "%s: %s %zu < %zu, a row", what, name, pitch, row);
}

// unit_name: "a component" (a quarter of the texel) or "a texel"
int check_pitch_aligned(cfhip_ctx* ctx, const char* what, const char* name, size_t pitch, size_t unit, const char* unit_name)
{
	if (pitch % unit)
		return fail(ctx, CFHIP_E_INVALID, "%s: %s %zu not aligned to %s (%zu bytes)", what, name, pitch, unit_name, unit);
	return CFHIP_OK;
}

int check_item_given(cfhip_ctx* ctx, const char* what, const char* name, uint32_t i, const void* p)
{
	return p ? CFHIP_OK : fail(ctx, CFHIP_E_INVALID, "%s: %s[%u] is NULL", what, name, i);
}

int check_item_aligned(cfhip_ctx* ctx, const char* what, const char* name, uint32_t i, const void* p, size_t unit,
	const char* unit_name)
{
	if ((uintptr_t)p % unit)
		return fail(ctx, CFHIP_E_INVALID, "%s: %s[%u] not aligned to %s (%zu bytes)", what, name, i, unit_name, unit);
	return CFHIP_OK;
}

// level k of layer l in the levels list of a generated chain: RGBA32F, `per` listed levels a layer
int check_chain_level(cfhip_ctx* ctx, const char* what, void* const* levels, uint32_t per, uint32_t l, uint32_t k)
{
	const size_t i = (size_t)l*per + (k - 1u);
	if (!levels[i])
		return fail(ctx, CFHIP_E_INVALID, "%s: levels[%zu] (layer %u, level %u) is NULL", what, i, l, k);
	if ((uintptr_t)levels[i] % 16u)
		return fail(ctx, CFHIP_E_INVALID, "%s: levels[%zu] is not aligned to a texel (16 bytes)", what, i);
	return CFHIP_OK;
}

int check_flags(cfhip_ctx* ctx, const char* what, uint32_t flags, uint32_t known)
{
	return (flags & ~known) ? fail(ctx, CFHIP_E_INVALID, "%s: params->flags 0x%x: unknown", what, flags) : CFHIP_OK;
}

// the alpha threshold of the passes that split texels at alpha > t
int check_threshold(cfhip_ctx* ctx, const char* what, float t)
{
	if (!(t >= 0.0f && t < 1.0f))
		return fail(ctx, CFHIP_E_INVALID, "%s: params->alpha_threshold %g outside [0, 1)", what, (double)t);
	return CFHIP_OK;
}

// the six faces of a cube, each face_size^2 tightly packed RGBA32F
int check_faces(cfhip_ctx* ctx, const char* what, const void* const* faces, uint32_t face_size)
{
	CF_TRY(check_given(ctx, what, "faces", faces));
	if (!face_size || face_size > CFENV_MAX_FACE)
		return fail(ctx, CFHIP_E_INVALID, "%s: face_size is 1 to %u, not %u", what, CFENV_MAX_FACE, face_size);
	for (uint32_t f = 0; f < 6u; ++f) {
		CF_TRY(check_item_given(ctx, what, "faces", f, faces[f]));
		CF_TRY(check_item_aligned(ctx, what, "faces", f, faces[f], 16u, "a texel"));
	}
	return CFHIP_OK;
}

// ---- the stream codecs' stage logs (estimator, deflate, inflate, LZ4, PNG: the sections far below) ------------------
// A family of calls that keeps a stage log: the public names its cfhip_*_stage_ms answers for (the log's owner tag), the
// kernel name its calls leave in last_kernel, and the shape of its event pairs (csrc/stage_log.h).
struct StageFamily {
	const char* calls;
	const char* kernel;
	size_t head, per_slice, tail;
};
const StageFamily kLzSizeStages = {"cfhip_lz_size", "cfhip_lz_match_kernel", 0, CFLZ_STAGES, 0};
const StageFamily kDeflateStages = {"cfhip_deflate", "cfhip_deflate_emit_kernel", 0, CFDF_STAGES, 0};
const StageFamily kInflateStages = {"cfhip_inflate", "cfhip_inflate_decode_kernel", 0, CFINF_STAGES, 0};
const StageFamily kLz4EncodeStages = {"cfhip_lz4_encode", "cfhip_lz4_emit_kernel", 0, CFLZ4_STAGES - 1, 1};
const StageFamily kLz4DecodeStages = {"cfhip_lz4_decode", "cfhip_lz4_block_kernel", CFLZ4_DSTAGES, 0, 0};
// filter; the encoder's stages per slice (png_run calls deflate_run, the log stays the writer's); crc, final
const StageFamily kPngStages = {"cfhip_png_encode", "cfhip_png_filter_kernel", 1, CFDF_STAGES, 2};

// begin_call of an entry point of family f: the log is f's, empty, and starts at the call's next event pair.  Entry
// points alone open it -- the *_run routines below them serve several families, and a search that owns no log.
void begin_call(cfhip_ctx* ctx, hipStream_t stream, const StageFamily& f)
{
	begin_call(ctx, stream, f.kernel);
	ctx->stages = StageLog{f.calls, ctx->events_used, 0, f.head, f.per_slice, f.tail};
}

// n event pairs into ev[0 .. 2n), counted into the open stage log
int take_event_pairs(cfhip_ctx* ctx, hipEvent_t* ev, size_t n)
{
	for (size_t k = 0; k < n; ++k) {
		const int rc = next_event_pair(ctx, &ev[2*k], &ev[2*k + 1]);
		if (rc != CFHIP_OK)
			return rc;
	}
	if (ctx->stages.owner)
		ctx->stages.pairs += n;
	return CFHIP_OK;
}

// cfhip_*_stage_ms of family f: the open log's pairs summed by stage into ms[0 .. n).  The log is f's last call's while
// f owns it and last_kernel still holds what that call wrote there.  Every call that times its launches passes through
// begin_call, which closes the log; mip generation (2-D, array, 3-D) and resize do not -- their launches are untimed and
// they leave the event state, the log and last_kernel alone, so f's log stays readable across them.  The comparison
// stays for a call that wrote last_kernel past begin_call.
int stage_ms(cfhip_ctx* ctx, const StageFamily& f, const char* what, float* ms, size_t n)
{
	const size_t stages = f.head + f.per_slice + f.tail;
	if (!ctx || !ms || n > stages)
		return CFHIP_E_INVALID;
	std::lock_guard<std::mutex> guard(ctx->lock);
	const StageLog& log = ctx->stages;
	if (log.owner != f.calls || ctx->last_kernel != f.kernel || !stage_log_valid(log, ctx->events_used))
		return fail(ctx, CFHIP_E_INVALID, "%s: the last call on this context was no %s*", what, f.calls);
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->events_stream));
	float sum[16] = {};
	static_assert(CFPNG_STAGES <= 16 && CFLZ4_STAGES <= 16, "the longest family's stages fit");
	for (size_t i = 0; i < log.pairs; ++i) {
		float t = 0.0f;
		HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->events[log.first + 2*i], ctx->events[log.first + 2*i + 1]));
		sum[stage_log_stage(log, i)] += t;
	}
	std::copy(sum, sum + n, ms);
	return CFHIP_OK;
}

// Where a host call's result words lie in d_out: behind `bytes` of output, 256-byte aligned; they take 256 bytes.
size_t result_offset(size_t bytes)
{
	return (bytes + 255u)/256u*256u;
}

// The tail of a host call whose output's size the device decides: the result words at d_res, then exactly bytes_out
// bytes (never more than `bound`) from d_from into out, the lease's end, *result.
template <class Result>
int download_sized(cfhip_ctx* ctx, StagingLease& lease, const char* what, const void* d_res, const void* d_from, size_t bound,
	void* out, Result* result)
{
	Result res;
	HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, lease.stream));
	HIP_TRY(ctx, hipStreamSynchronize(lease.stream));
	if (res.bytes_out > bound)
		return fail(ctx, CFHIP_E_DEVICE, "%s: %llu bytes exceed the bound", what, (unsigned long long)res.bytes_out);
	HIP_TRY(ctx, hipMemcpyAsync(out, d_from, (size_t)res.bytes_out, hipMemcpyDeviceToHost, lease.stream));
	const int rc = lease.done(true);
	if (rc == CFHIP_OK)
		*result = res;
	return rc;
}

// Its twin for the decoders, whose output's size the caller knows: the bytes come only where the status is 0 (no
// error).  The caller turns *result's status into the call's verdict.
template <class Result>
int download_checked(cfhip_ctx* ctx, StagingLease& lease, const void* d_res, const void* d_from, size_t out_bytes, void* out,
	Result* result)
{
	Result res;
	HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, lease.stream));
	HIP_TRY(ctx, hipStreamSynchronize(lease.stream));
	if (res.status == 0)
		HIP_TRY(ctx, hipMemcpyAsync(out, d_from, out_bytes, hipMemcpyDeviceToHost, lease.stream));
	const int rc = lease.done(true);
	if (rc == CFHIP_OK)
		*result = res;
	return rc;
}

// One launch for many surfaces (same format / pixel type): workgroups are numbered across
// the surfaces, the kernel resolves its surface with a uniform binary search (cf_resolve).
int batched_launch(cfhip_ctx* ctx, StagingLease& lease, const std::vector<cf_kparams>& kps, const cfhip_params& p,
	int pixel_type)
{
	const hipStream_t stream = lease.stream;
	if (kps.size() == 1)
		return timed_launch(ctx, kps[0], p, pixel_type, stream);
	if (is_std_format(p.format)) {
		// bandwidth-bound per-pixel work with no workgroup tiling to share: one launch each
		for (const cf_kparams& k : kps) {
			const int rc = timed_launch(ctx, k, p, pixel_type, stream);
			if (rc != CFHIP_OK)
				return rc;
		}
		return CFHIP_OK;
	}
	std::vector<cf_batch_entry> entries(kps.size());
	uint32_t wg = 0, per_wg;
	// (the launch shape is chosen for the first surface's row length; the launch below repeats the choice)
	int rc = blocks_per_wg(ctx, p, kps[0].quality, kps[0].bx, &per_wg);
	if (rc != CFHIP_OK)
		return rc;
	for (size_t i = 0; i < kps.size(); ++i) {
		cf_batch_entry& e = entries[i];
		e.src = kps[i].src; e.out = kps[i].out; e.pitch = kps[i].pitch;
		e.width = kps[i].width; e.height = kps[i].height; e.bx = kps[i].bx; e.by = kps[i].by;
		e.wgx = (kps[i].bx + per_wg - 1)/per_wg;
		e.wg_begin = wg;
		wg += e.wgx*kps[i].by;
	}
	const size_t bytes = entries.size()*sizeof(cf_batch_entry);
	rc = lease.acquire();
	if (rc != CFHIP_OK)
		return rc;
	rc = reserve(ctx, &ctx->d_batch, &ctx->batch_cap, bytes);
	if (rc != CFHIP_OK)
		return rc;
	// pageable source: the runtime stages the copy before returning, so `entries` may die
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, entries.data(), bytes, hipMemcpyHostToDevice, stream));
	cf_kparams kp = kps[0];
	kp.batch = static_cast<const cf_batch_entry*>(ctx->d_batch);
	kp.nbatch = (uint32_t)entries.size();
	kp.total_wg = wg;
	return timed_launch(ctx, kp, p, pixel_type, stream);
}

// ---- pipelined host path ----------------------------------------
// A large host surface is cut into strips of whole block rows.  Host threads STAGE strip k+1
// into a pinned slot -- a row gather that accepts any (also negative: bottom-up FreeImage
// bitmaps) pitch, fused for RGBA32F sources of 8-bit formats with the reference's float ->
// UNORM8 quantisation (toColorBlock, S3tcConverter.cpp:97-111; 4x less PCIe traffic) -- while
// strip k is uploaded and encoded on the stream.  Replaces the per-surface serial
// convert-upload-encode of Converter::convert (Converter.cpp:521-589).

// formats whose kernels consume 8-bit texels for UNorm: their RGBA32F loader is cf_unorm8
bool takes_unorm8(const cfhip_params& p)
{
	if (p.type != CFHIP_TYPE_UNORM || is_std_format(p.format))
		return false;
	if (p.format == CFHIP_FORMAT_EAC_R11 || p.format == CFHIP_FORMAT_EAC_R11G11 ||
		p.format == CFHIP_FORMAT_BC6H)
		return false;
	return true;
}

inline uint8_t host_unorm8(float f)
{
	// (uint8)std::round(clamp(f,0,1)*255); NaN -> 0 like the device conversion
	if (!(f > 0.0f))
		return 0;
	f = f > 1.0f ? 1.0f : f;
	// roundf, like cf_unorm8 on the device and std::round in the reference: f*255 + 0.5 rounds UP
	// in float arithmetic for f*255 = 0.5 - 2^-25, where round() says 0
	return (uint8_t)roundf(f*255.0f);
}

// 8 floats -> 8 UNORM8 bytes with the arithmetic of host_unorm8, exactly: clamp (NaN -> 0: maxps returns its
// second operand when one is NaN), times 255, round half away from zero as trunc(x) + (x - trunc(x) >= 0.5)
// (x + 0.5 would round up at x = 0.5 - 2^-25), all exact in float for x in [0, 255].
__attribute__((target("avx2")))
void quantise_row_avx2(const float* f, uint8_t* d, size_t nv)
{
	const __m256 zero = _mm256_setzero_ps(), one = _mm256_set1_ps(1.0f), k255 = _mm256_set1_ps(255.0f),
		half = _mm256_set1_ps(0.5f);
	size_t i = 0;
	for (; i + 32 <= nv; i += 32) {
		__m256i r[4];
		for (int k = 0; k < 4; ++k) {
			__m256 v = _mm256_loadu_ps(f + i + 8*k);
			v = _mm256_min_ps(_mm256_max_ps(v, zero), one);
			v = _mm256_mul_ps(v, k255);
			const __m256 t = _mm256_round_ps(v, _MM_FROUND_TO_ZERO | _MM_FROUND_NO_EXC);
			const __m256 up = _mm256_and_ps(_mm256_cmp_ps(_mm256_sub_ps(v, t), half, _CMP_GE_OQ), one);
			r[k] = _mm256_cvttps_epi32(_mm256_add_ps(t, up));
		}
		// 32 x i32 -> 32 x u8 in order: the packs work per 128-bit lane, one permute restores the order
		const __m256i p01 = _mm256_packus_epi32(r[0], r[1]), p23 = _mm256_packus_epi32(r[2], r[3]);
		__m256i b = _mm256_packus_epi16(p01, p23);
		b = _mm256_permutevar8x32_epi32(b, _mm256_setr_epi32(0, 4, 1, 5, 2, 6, 3, 7));
		_mm256_storeu_si256(reinterpret_cast<__m256i*>(d + i), b);
	}
	for (; i < nv; ++i)
		d[i] = host_unorm8(f[i]);
}

void stage_rows(const cfhip_surface& s, uint32_t y0, uint32_t y1, size_t row_bytes, bool quantise,
	uint8_t* dst, size_t dst_pitch)
{
	static const bool avx2 = __builtin_cpu_supports("avx2");
	const uint8_t* base = static_cast<const uint8_t*>(s.pixels);
	for (uint32_t y = y0; y < y1; ++y) {
		const uint8_t* src = base + (ptrdiff_t)y*s.row_pitch_bytes;
		uint8_t* d = dst + (size_t)(y - y0)*dst_pitch;
		if (!quantise)
			std::memcpy(d, src, row_bytes);
		else {
			const float* f = reinterpret_cast<const float*>(src);
			const size_t nv = (size_t)s.width*4u;
			if (avx2)
				quantise_row_avx2(f, d, nv);
			else
				for (size_t i = 0; i < nv; ++i)
					d[i] = host_unorm8(f[i]);
		}
	}
}

// host threads this process may really use: the scheduler affinity capped by the cgroup CPU quota
// (hardware_concurrency() reports the machine, not the container's share)
unsigned usable_cpus()
{
	unsigned n = std::max(1u, std::thread::hardware_concurrency());
	cpu_set_t set;
	if (sched_getaffinity(0, sizeof(set), &set) == 0) {
		const int c = CPU_COUNT(&set);
		if (c > 0)
			n = std::min(n, (unsigned)c);
	}
	if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
		char a[32] = {0};
		long long period = 0;
		if (std::fscanf(f, "%31s %lld", a, &period) == 2 && std::strcmp(a, "max") != 0 && period > 0) {
			const long long quota = std::atoll(a);
			if (quota > 0)
				n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, quota/period));
		}
		std::fclose(f);
	}
	return std::max(1u, n);
}

// Strips of whole block rows flow through four overlapped stages: host threads gather (and quantise) strip
// k+2 into a pinned slot | the upload stream copies strip k+1 | the launch stream encodes strip k | the
// download stream returns the payload of strip k-1 into a pinned landing buffer.  Three pinned slots; events
// order slot reuse (pin_free), upload -> kernel (up_done) and kernel -> download (one pair per strip).  An error return
// from the middle leaves copies queued on the copy streams that still read and write the pinned slots: the lease drains
// them before the error goes to the caller, so the next call can never stage into a slot an old upload is reading.
int encode_strip_pipeline(cfhip_ctx* ctx, StagingLease& lease, const cfhip_surface& s, const cfhip_params& p)
{
	const hipStream_t stream = lease.stream;
	int fbw, fbh;
	block_dims(p.format, &fbw, &fbh);
	const int bs = unit_bytes(p.format, p.type);
	const bool quantise = s.pixel_type == CFHIP_PIXEL_RGBA32F && takes_unorm8(p);
	const int dev_type = quantise ? CFHIP_PIXEL_RGBA8 : s.pixel_type;
	const size_t dev_row = (size_t)s.width*pixel_bytes(dev_type);
	const size_t src_row = (size_t)s.width*pixel_bytes(s.pixel_type);
	const uint32_t bx = (s.width + (uint32_t)fbw - 1u)/(uint32_t)fbw;
	const uint32_t by = (s.height + (uint32_t)fbh - 1u)/(uint32_t)fbh;
	const size_t out_bytes = (size_t)bx*by*(size_t)bs;
	// strips of whole block rows, ~4 MB of device pixels each, at least 8 of them: short enough that the
	// pipeline's fill (first strip staged and uploaded before anything is encoded) and drain stay small
	uint32_t strip_brows = (uint32_t)std::max<size_t>(1, ((size_t)4 << 20)/(dev_row*(size_t)fbh));
	strip_brows = std::min(strip_brows, std::max(1u, by/8u));
	if (is_std_format(p.format))
		strip_brows = (strip_brows + 3u) & ~3u;   // every strip's output stays 4-byte aligned
	const size_t strip_bytes = (size_t)strip_brows*(size_t)fbh*dev_row;
	int rc = lease.acquire();
	if (rc != CFHIP_OK) return rc;
	rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, dev_row*(size_t)s.height);
	if (rc != CFHIP_OK) return rc;
	rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, out_bytes);
	if (rc != CFHIP_OK) return rc;
	constexpr int NS = cfhip_ctx::kPinSlots;
	if (!ctx->up_stream) {
		HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking));
		HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking));
		for (int i = 0; i < NS; ++i) {
			HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pin_free[i], hipEventDisableTiming));
			HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->up_done[i], hipEventDisableTiming));
		}
	}
	if (ctx->pin_cap < strip_bytes) {
		for (int i = 0; i < NS; ++i) {
			if (ctx->h_pin[i]) { HIP_TRY(ctx, hipHostFree(ctx->h_pin[i])); ctx->h_pin[i] = nullptr; }
			HIP_TRY(ctx, hipHostMalloc(&ctx->h_pin[i], strip_bytes, hipHostMallocDefault));
		}
		ctx->pin_cap = strip_bytes;
	}
	// The payload lands in a RING of kOutSlots pinned strips (round 6; it used to be one pinned buffer as large as the
	// largest payload the context had ever produced, never shrunk: 256 MB of locked memory after one 16k x 16k BC7
	// surface).  A strip's slot is reused once this thread has copied it on to the caller's buffer.  When the pinned
	// allocation fails the downloads go straight into the caller's pageable buffer -- slower (the runtime stages them),
	// never an error.
	constexpr int NO = cfhip_ctx::kOutSlots;
	const size_t strip_out = (((size_t)strip_brows*bx*(size_t)bs) + 255u) & ~(size_t)255u;
	if (ctx->h_out_cap < strip_out*(size_t)NO) {
		if (ctx->h_out) { HIP_TRY(ctx, hipHostFree(ctx->h_out)); ctx->h_out = nullptr; ctx->h_out_cap = 0; }
		// (CFHIP_NO_PINNED_OUT: test hook -- behave as if the allocation had failed)
		if (!std::getenv("CFHIP_NO_PINNED_OUT") &&
			hipHostMalloc(&ctx->h_out, strip_out*(size_t)NO, hipHostMallocDefault) == hipSuccess)
			ctx->h_out_cap = strip_out*(size_t)NO;
		else {
			(void)hipGetLastError();
			ctx->h_out = nullptr;
		}
	}
	if (!ctx->pool) {
		ctx->pool = new (std::nothrow) cf_host_pool;
		if (!ctx->pool)
			return fail(ctx, CFHIP_E_DEVICE, "host worker pool: out of memory");
		ctx->pool->start(std::min(32u, usable_cpus()) - 1u);      // the calling thread is a worker too
	}
	const unsigned nthreads = (unsigned)ctx->pool->threads.size() + 1u;
	uint32_t slot_used[NS] = {0, 0, 0};
	uint8_t* hout = static_cast<uint8_t*>(ctx->h_out);
	uint8_t* user_out = static_cast<uint8_t*>(s.out);
	// payload that has landed in h_out is copied to the caller's buffer by this thread while it waits for a slot
	struct Landed { size_t off, bytes, ring; hipEvent_t ev; };
	std::vector<Landed> landing;
	size_t landed = 0;
	size_t ev_used = 0;
	auto next_event = [&](hipEvent_t* ev) -> int {
		if (ev_used == ctx->strip_events.size()) {
			hipEvent_t e;
			HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
			ctx->strip_events.push_back(e);
		}
		*ev = ctx->strip_events[ev_used++];
		return CFHIP_OK;
	};
	{
		// the copy streams start after whatever the launch stream was asked to wait for (the lease's acquire)
		hipEvent_t order;
		rc = next_event(&order);
		if (rc != CFHIP_OK) return rc;
		HIP_TRY(ctx, hipEventRecord(order, stream));
		HIP_TRY(ctx, hipStreamWaitEvent(ctx->up_stream, order, 0));
		HIP_TRY(ctx, hipStreamWaitEvent(ctx->down_stream, order, 0));
	}
	auto drain = [&](bool all) -> int {
		while (landed < landing.size()) {
			const Landed& l = landing[landed];
			if (all)
				HIP_TRY(ctx, hipEventSynchronize(l.ev));
			else if (hipEventQuery(l.ev) != hipSuccess)
				break;
			if (hout)
				std::memcpy(user_out + l.off, hout + l.ring, l.bytes);
			++landed;
		}
		return CFHIP_OK;
	};
	uint32_t k = 0;
	for (uint32_t br0 = 0; br0 < by; br0 += strip_brows, ++k) {
		const uint32_t br1 = std::min(by, br0 + strip_brows);
		const uint32_t y0 = br0*(uint32_t)fbh, y1 = std::min(s.height, br1*(uint32_t)fbh);
		const int slot = (int)(k % (uint32_t)NS);
		if (slot_used[slot])
			HIP_TRY(ctx, hipEventSynchronize(ctx->pin_free[slot]));
		uint8_t* pin = static_cast<uint8_t*>(ctx->h_pin[slot]);
		// stage rows [y0, y1) with the pool
		const uint32_t rows = y1 - y0;
		const unsigned nt = std::min<unsigned>(nthreads, rows);
		ctx->pool->run(nt, [&](unsigned t) {
			const uint32_t a = y0 + (uint32_t)((unsigned long long)rows*t/nt);
			const uint32_t b = y0 + (uint32_t)((unsigned long long)rows*(t + 1)/nt);
			stage_rows(s, a, b, src_row, quantise, pin + (size_t)(a - y0)*dev_row, dev_row);
		});
		uint8_t* dsrc = static_cast<uint8_t*>(ctx->d_src) + (size_t)y0*dev_row;
		HIP_TRY(ctx, hipMemcpyAsync(dsrc, pin, (size_t)rows*dev_row, hipMemcpyHostToDevice, ctx->up_stream));
		HIP_TRY(ctx, hipEventRecord(ctx->pin_free[slot], ctx->up_stream));
		HIP_TRY(ctx, hipEventRecord(ctx->up_done[slot], ctx->up_stream));
		slot_used[slot] = 1;
		HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->up_done[slot], 0));
		cf_kparams kp;
		const size_t out_off = (size_t)br0*bx*(size_t)bs, out_n = (size_t)(br1 - br0)*bx*(size_t)bs;
		fill_kparams(kp, p, dsrc, static_cast<uint8_t*>(ctx->d_out) + out_off, (long long)dev_row, s.width, rows);
		rc = timed_launch(ctx, kp, p, dev_type, stream);
		if (rc != CFHIP_OK)
			return rc;
		// the strip's payload leaves on the download stream as soon as its kernel is done
		hipEvent_t enc, down;
		rc = next_event(&enc);
		if (rc != CFHIP_OK) return rc;
		rc = next_event(&down);
		if (rc != CFHIP_OK) return rc;
		HIP_TRY(ctx, hipEventRecord(enc, stream));
		HIP_TRY(ctx, hipStreamWaitEvent(ctx->down_stream, enc, 0));
		// the ring slot of strip k held strip k - NO: that one must have gone on to the caller's buffer
		while (hout && landed + (size_t)NO <= (size_t)k) {
			const Landed& l = landing[landed];
			HIP_TRY(ctx, hipEventSynchronize(l.ev));
			std::memcpy(user_out + l.off, hout + l.ring, l.bytes);
			++landed;
		}
		const size_t ring = (size_t)(k % (uint32_t)NO)*strip_out;
		HIP_TRY(ctx, hipMemcpyAsync(hout ? hout + ring : user_out + out_off, static_cast<uint8_t*>(ctx->d_out) + out_off, out_n,
			hipMemcpyDeviceToHost, ctx->down_stream));
		HIP_TRY(ctx, hipEventRecord(down, ctx->down_stream));
		landing.push_back({out_off, out_n, ring, down});
		rc = drain(false);
		if (rc != CFHIP_OK)
			return rc;
	}
	rc = drain(true);
	HIP_TRY(ctx, hipStreamSynchronize(stream));
	return rc;
}


// ---- decoding (csrc/decode.hip) ------------------------------------------------------------------
// decoded texel layout of a block (format, type) pair: false for the standard formats and the illegal pairs
bool decoded_layout(int format, int type, int* layout, int* texel_bytes)
{
	if (is_std_format(format) || !block_bytes(format) || !type_valid(format, type))
		return false;
	const bool sn = type == CFHIP_TYPE_SNORM;
	int l = CFHIP_LAYOUT_RGBA8, tb = 4;
	switch (format) {
		case CFHIP_FORMAT_BC4: l = sn ? CFHIP_LAYOUT_R8_SNORM : CFHIP_LAYOUT_R8; tb = 1; break;
		case CFHIP_FORMAT_BC5: l = sn ? CFHIP_LAYOUT_RG8_SNORM : CFHIP_LAYOUT_RG8; tb = 2; break;
		case CFHIP_FORMAT_EAC_R11: l = sn ? CFHIP_LAYOUT_R16_SNORM : CFHIP_LAYOUT_R16; tb = 2; break;
		case CFHIP_FORMAT_EAC_R11G11: l = sn ? CFHIP_LAYOUT_RG16_SNORM : CFHIP_LAYOUT_RG16; tb = 4; break;
		case CFHIP_FORMAT_BC6H: l = CFHIP_LAYOUT_RGBA16F; tb = 8; break;
		default:
			if (format >= CFHIP_FORMAT_ASTC_4x4 && type == CFHIP_TYPE_UFLOAT) {
				l = CFHIP_LAYOUT_RGBA16F;
				tb = 8;
			}
			break;
	}
	*layout = l;
	*texel_bytes = tb;
	return true;
}

struct DecodeGeom {
	int layout, texel_bytes, bw, bh, bb;
	uint32_t bx, by;
	size_t payload_bytes;
};

// the checks every decode entry point makes before anything is enqueued
int decode_check(cfhip_ctx* ctx, const char* what, int format, int type, const void* blocks, uint32_t width,
	uint32_t height, bool sse, DecodeGeom* g)
{
	if (!decoded_layout(format, type, &g->layout, &g->texel_bytes))
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: (format %d, type %d) has no decoded layout", what, format, type);
	if (sse && g->layout != CFHIP_LAYOUT_RGBA8 && g->layout != CFHIP_LAYOUT_R8 && g->layout != CFHIP_LAYOUT_RG8)
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: SSE covers the RGBA8, R8 and RG8 layouts only (format %d, type %d)",
			what, format, type);
	if (!blocks)
		return fail(ctx, CFHIP_E_INVALID, "%s: blocks is NULL", what);
	if (!width || !height)
		return fail(ctx, CFHIP_E_INVALID, "%s: empty surface %ux%u", what, width, height);
	block_dims(format, &g->bw, &g->bh);
	g->bb = block_bytes(format);
	g->bx = (width + (uint32_t)g->bw - 1)/(uint32_t)g->bw;
	g->by = (height + (uint32_t)g->bh - 1)/(uint32_t)g->bh;
	g->payload_bytes = (size_t)g->bx*g->by*(size_t)g->bb;
	// launch geometry: ASTC runs one workgroup row per block row (grid y), the 4x4 kernels one lane per block
	if ((format >= CFHIP_FORMAT_ASTC_4x4 && g->by > 65535u) || (uint64_t)g->bx*g->by > (1ull << 38))
		return fail(ctx, CFHIP_E_INVALID, "%s: surface %ux%u too large for one launch", what, width, height);
	return CFHIP_OK;
}

// one decode (or decode + SSE) launch, timed like every encode launch (cfhip_last_kernel_ms / profiling)
int decode_launch(cfhip_ctx* ctx, int format, int type, const DecodeGeom& g, const void* blocks, void* out,
	size_t out_pitch, const void* ref, size_t ref_pitch, uint32_t width, uint32_t height, unsigned long long* acc,
	bool sse, hipStream_t stream)
{
	const bool astc = format >= CFHIP_FORMAT_ASTC_4x4;
	begin_call(ctx, stream, sse ? (astc ? "cfhip_decode_sse_astc_kernel" : "cfhip_decode_sse_block_kernel")
		: (astc ? "cfhip_decode_astc_kernel" : "cfhip_decode_block_kernel"));
	const uintptr_t op = sse ? (uintptr_t)ref : (uintptr_t)out;
	const size_t pitch = sse ? ref_pitch : out_pitch;
	// decode: 16-byte row stores need a 16-byte aligned output; SSE: word loads of the reference need 4 bytes
	const int align = sse ? 4 : 16;
	const int out_vec = (op % align == 0 && pitch % align == 0) ? 1 : 0;
	const int blk_vec = ((uintptr_t)blocks % (uintptr_t)g.bb == 0) ? 1 : 0;
	return timed(ctx, stream, "decode", [&] {
		return cfhip_launch_decode(format, type, blocks, blk_vec, out, out_pitch, ref, ref_pitch, out_vec,
			width, height, g.bx, g.by, g.bw, g.bh, acc, sse ? 1 : 0, stream);
	});
}

// ---- quality metrics (csrc/compare.hip) -----------------------------------------------------------
// What one compare call runs and where its device scratch lies: the decoded surface of the SSIM pass, then the
// Pass A partials (16 doubles per workgroup), then the SSIM partials (4 doubles per workgroup).
struct CompareGeom {
	DecodeGeom g;
	int ref_bytes;
	unsigned cmask;
	bool hdr, ssim;
	uint64_t na, nb;
	uint32_t windows;
	size_t pa_off, pb_off, scratch_bytes;
};

size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// the checks every compare entry point makes before anything is enqueued
int compare_check(cfhip_ctx* ctx, const char* what, int format, int type, const void* blocks, uint32_t width,
	uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch, const uint8_t* mask, unsigned flags,
	const void* result, const void* block_errors, size_t block_errors_capacity, CompareGeom* c)
{
	int rc = decode_check(ctx, what, format, type, blocks, width, height, false, &c->g);
	if (rc != CFHIP_OK)
		return rc;
	if (!ref || !result)
		return fail(ctx, CFHIP_E_INVALID, "%s: NULL reference or result", what);
	switch (ref_pixel_type) {
		case CFHIP_PIXEL_RGBA8: c->ref_bytes = 4; break;
		case CFHIP_PIXEL_RGBA32F: c->ref_bytes = 16; break;
		case CFHIP_PIXEL_RGBA16F: c->ref_bytes = 8; break;
		default: return fail(ctx, CFHIP_E_INVALID, "%s: reference pixel type %d", what, ref_pixel_type);
	}
	if (ref_pitch < (size_t)width*(size_t)c->ref_bytes)
		return fail(ctx, CFHIP_E_INVALID, "%s: reference pitch %zu < %zu", what, ref_pitch,
			(size_t)width*(size_t)c->ref_bytes);
	if (flags & ~CFHIP_COMPARE_SSIM)
		return fail(ctx, CFHIP_E_INVALID, "%s: unknown flags 0x%x", what, flags);
	const int l = c->g.layout;
	const unsigned lay = (l == CFHIP_LAYOUT_RGBA8 || l == CFHIP_LAYOUT_RGBA16F) ? 15u :
		((l == CFHIP_LAYOUT_R8 || l == CFHIP_LAYOUT_R8_SNORM || l == CFHIP_LAYOUT_R16 || l == CFHIP_LAYOUT_R16_SNORM)
			? 1u : 3u);
	unsigned m = 15u;
	if (mask)
		m = (mask[0] ? 1u : 0u) | (mask[1] ? 2u : 0u) | (mask[2] ? 4u : 0u) | (mask[3] ? 8u : 0u);
	c->cmask = lay & m;
	c->hdr = l == CFHIP_LAYOUT_RGBA16F;
	const uint64_t nblk = (uint64_t)c->g.bx*c->g.by;
	if (block_errors && block_errors_capacity < nblk)
		return fail(ctx, CFHIP_E_CAPACITY, "%s: block_errors_capacity %zu < %llu blocks", what,
			block_errors_capacity, (unsigned long long)nblk);
	c->na = cfhip_compare_partials(format, width, height, c->g.bx, c->g.by, &c->nb);
	c->ssim = (flags & CFHIP_COMPARE_SSIM) && !c->hdr && c->nb > 0 && c->cmask;
	if (!c->ssim)
		c->nb = 0;
	c->windows = 0;
	if (c->ssim) {
		const uint64_t win = (uint64_t)(width - 10u)*(height - 10u);
		if (win > 0xFFFFFFFFull || (height - 10u + 15u)/16u > 65535u)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %ux%u too large for SSIM", what, width, height);
		c->windows = (uint32_t)win;
	}
	const size_t dec = c->ssim ? (size_t)width*height*(size_t)c->g.texel_bytes : 0;
	c->pa_off = align16(dec);
	c->pb_off = c->pa_off + (size_t)c->na*16u*sizeof(double);
	c->scratch_bytes = c->pb_off + (size_t)c->nb*4u*sizeof(double);
	return CFHIP_OK;
}

// the normalised 11-tap Gaussian of the SSIM window (sigma 1.5), in double, rounded to float
const float* ssim_taps()
{
	static float taps[11];
	static std::once_flag once;
	std::call_once(once, [] {
		double w[11], s = 0.0;
		for (int k = -5; k <= 5; ++k)
			s += w[k + 5] = std::exp(-(double)(k*k)/4.5);
		for (int k = 0; k < 11; ++k)
			taps[k] = (float)(w[k]/s);
	});
	return taps;
}

// Pass A, the SSIM pass (decode into scratch + window statistics) and the final reduction, timed as one span
int compare_enqueue(cfhip_ctx* ctx, int format, int type, const CompareGeom& c, const void* blocks, const void* ref,
	int ref_pixel_type, size_t ref_pitch, uint32_t width, uint32_t height, uint8_t* scratch,
	cfhip_compare_result* result, float* block_errors, hipStream_t stream)
{
	begin_call(ctx, stream, format >= CFHIP_FORMAT_ASTC_4x4 ? "cfhip_compare_astc_kernel" : "cfhip_compare_block_kernel");
	const DecodeGeom& g = c.g;
	const int blk_vec = ((uintptr_t)blocks % (uintptr_t)g.bb == 0) ? 1 : 0;
	double* pa = reinterpret_cast<double*>(scratch + c.pa_off);
	double* pb = c.ssim ? reinterpret_cast<double*>(scratch + c.pb_off) : nullptr;
	return timed(ctx, stream, "compare", [&] {
		hipError_t e = cfhip_launch_compare(format, type, blocks, blk_vec, ref, ref_pixel_type, ref_pitch, width, height,
			g.bx, g.by, g.bw, g.bh, c.cmask, block_errors, pa, stream);
		if (e == hipSuccess && c.ssim) {
			const size_t dec_pitch = (size_t)width*(size_t)g.texel_bytes;
			e = cfhip_launch_decode(format, type, blocks, blk_vec, scratch, dec_pitch, nullptr, 0,
				dec_pitch % 16u == 0 ? 1 : 0, width, height, g.bx, g.by, g.bw, g.bh, nullptr, 0, stream);
			if (e == hipSuccess) {
				const double range = (g.layout == CFHIP_LAYOUT_R8_SNORM || g.layout == CFHIP_LAYOUT_RG8_SNORM ||
					g.layout == CFHIP_LAYOUT_R16_SNORM || g.layout == CFHIP_LAYOUT_RG16_SNORM) ? 2.0 : 1.0;
				e = cfhip_launch_ssim(scratch, dec_pitch, g.layout, ref, ref_pixel_type, ref_pitch, width, height, c.cmask,
					ssim_taps(), range, pb, stream);
			}
		}
		if (e == hipSuccess)
			e = cfhip_launch_compare_final(pa, c.na, pb, c.nb, c.cmask, c.hdr ? 1 : 0, c.windows,
				(uint64_t)width*height, result, stream);
		return e;
	});
}

} // namespace

extern "C" {

int cfhip_abi_version(void)
{
	return CFHIP_ABI_VERSION;
}

int cfhip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

cfhip_ctx* cfhip_create(int device_id, unsigned flags, int* err)
{
	(void)flags;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) {
		int code = (e != hipSuccess || n <= 0) ? CFHIP_E_NO_DEVICE : CFHIP_E_INVALID;
		fail(nullptr, code, "cfhip_create: device %d unavailable (%d HIP devices, %s)", device_id,
			n, hipGetErrorString(e));
		if (err) *err = code;
		return nullptr;
	}
	cfhip_ctx* ctx = new (std::nothrow) cfhip_ctx;
	if (!ctx) {
		if (err) *err = CFHIP_E_DEVICE;
		return nullptr;
	}
	ctx->device = device_id;
	if (hipSetDevice(device_id) != hipSuccess ||
		hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
		fail(nullptr, CFHIP_E_DEVICE, "cfhip_create: cannot create stream on device %d", device_id);
		delete ctx;
		if (err) *err = CFHIP_E_DEVICE;
		return nullptr;
	}
	if (err) *err = CFHIP_OK;
	return ctx;
}

void cfhip_destroy(cfhip_ctx* ctx)
{
	if (!ctx)
		return;
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) {
		(void)hipStreamSynchronize(ctx->stream);
		(void)hipStreamDestroy(ctx->stream);
	}
	for (hipEvent_t ev : ctx->events)
		(void)hipEventDestroy(ev);
	for (auto& kv : ctx->astc_tables)
		if (kv.second) (void)hipFree(kv.second);
	delete ctx->pool;
	if (ctx->up_stream) { (void)hipStreamSynchronize(ctx->up_stream); (void)hipStreamDestroy(ctx->up_stream); }
	if (ctx->down_stream) { (void)hipStreamSynchronize(ctx->down_stream); (void)hipStreamDestroy(ctx->down_stream); }
	for (int i = 0; i < cfhip_ctx::kPinSlots; ++i) {
		if (ctx->h_pin[i]) (void)hipHostFree(ctx->h_pin[i]);
		if (ctx->pin_free[i]) (void)hipEventDestroy(ctx->pin_free[i]);
		if (ctx->up_done[i]) (void)hipEventDestroy(ctx->up_done[i]);
	}
	for (hipEvent_t ev : ctx->strip_events)
		(void)hipEventDestroy(ev);
	if (ctx->h_out) (void)hipHostFree(ctx->h_out);
	if (ctx->staging_done) (void)hipEventDestroy(ctx->staging_done);
	if (ctx->group_up) (void)hipEventDestroy(ctx->group_up);
	if (ctx->d_batch) (void)hipFree(ctx->d_batch);
	if (ctx->d_mip3d) (void)hipFree(ctx->d_mip3d);
	if (ctx->d_pvrtc) (void)hipFree(ctx->d_pvrtc);
	if (ctx->d_lz) (void)hipFree(ctx->d_lz);
	if (ctx->d_rdo_keep) (void)hipFree(ctx->d_rdo_keep);
	if (ctx->d_png) (void)hipFree(ctx->d_png);
	if (ctx->d_src) (void)hipFree(ctx->d_src);
	if (ctx->d_out) (void)hipFree(ctx->d_out);
	delete ctx;
}

int cfhip_query(int format, int type, int* block_w, int* block_h, int* bytes)
{
	const int bs = unit_bytes(format, type);
	if (!bs || !type_valid(format, type))
		return CFHIP_E_UNSUPPORTED;
	int fbw, fbh;
	block_dims(format, &fbw, &fbh);
	if (block_w) *block_w = fbw;
	if (block_h) *block_h = fbh;
	if (bytes) *bytes = bs;
	return CFHIP_OK;
}

// Host-only introspection of the ASTC tables (tests/test_astc_tables.py compares them with the
// oracle's independently built tables): counts of canonical partitions, configs per class x alpha,
// and (mode | wq << 11) of every listed config.  Not part of the drop-in surface.
int cfhip_debug_astc_table_info(int bw, int bh, int* npart3, int* ncfg10, uint16_t* cfg_modes)
{
	const std::vector<uint8_t> blob = cfastc::build_blob(bw, bh);
	const cfastc::AstcBlobHeader* h = reinterpret_cast<const cfastc::AstcBlobHeader*>(blob.data());
	for (int t = 0; t < 3; ++t)
		npart3[t] = (int)h->npart[t];
	const cfastc::AstcCfgRec* cfgs = reinterpret_cast<const cfastc::AstcCfgRec*>(blob.data() + h->off_cfg);
	for (int i = 0; i < 10; ++i) {
		ncfg10[i] = blob[h->off_ncfg + i];
		for (int k = 0; k < 64; ++k)
			cfg_modes[i*64 + k] = k < ncfg10[i] ? (uint16_t)(cfgs[i*64 + k].mode | (cfgs[i*64 + k].wq << 11)) : 0xFFFF;
	}
	return (int)h->total;
}

// Host-only, read-only: the launch shape cfhip_astc_plan and the launcher give a bw x bh surface of bx blocks per
// row (tests/test_astc_cases.py enumerates the shapes; cfhip_astc_launch_shape in astc_encode.hip names the fields).
int cfhip_debug_astc_launch_shape(int bw, int bh, uint32_t quality, uint32_t hdr, uint32_t bx, uint32_t shape[4])
{
	const std::vector<uint8_t> blob = cfastc::build_blob(bw, bh);
	cfhip_astc_launch_shape(reinterpret_cast<const cfastc::AstcBlobHeader*>(blob.data()), quality, hdr, bx, shape);
	return CFHIP_OK;
}

int cfhip_shard_rows(uint32_t block_rows, int rank, int world, uint32_t* row_begin,
	uint32_t* row_end)
{
	if (world <= 0 || rank < 0 || rank >= world || !row_begin || !row_end)
		return CFHIP_E_INVALID;
	const unsigned long long r = (unsigned long long)block_rows;
	*row_begin = (uint32_t)(r*(unsigned long long)rank/(unsigned long long)world);
	*row_end = (uint32_t)(r*((unsigned long long)rank + 1ull)/(unsigned long long)world);
	return CFHIP_OK;
}

// sizes of one surface of a call, and the checks every entry point makes before it reads a texel
struct Item { size_t src_bytes, out_bytes, row_bytes; };
static int validate_surfaces(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n, const cfhip_params* params,
	bool device_mem, Item* items)
{
	const int bs = unit_bytes(params->format, params->type);
	int fbw, fbh;
	block_dims(params->format, &fbw, &fbh);
	for (size_t i = 0; i < n; ++i) {
		const cfhip_surface& s = surfaces[i];
		const size_t pb = pixel_bytes(s.pixel_type);
		if (!s.pixels || !s.out || !s.width || !s.height || !pb)
			return fail(ctx, CFHIP_E_INVALID, "surface %zu: bad pixels/out/size/pixel_type", i);
		const size_t row_bytes = (size_t)s.width*pb;
		const size_t apitch = (size_t)(s.row_pitch_bytes < 0 ? -s.row_pitch_bytes : s.row_pitch_bytes);
		if (apitch < row_bytes)
			return fail(ctx, CFHIP_E_INVALID, "surface %zu: |row pitch| %zu < row size %zu", i,
				apitch, row_bytes);
		const uint32_t bx = (s.width + (uint32_t)fbw - 1u)/(uint32_t)fbw;
		const uint32_t by = (s.height + (uint32_t)fbh - 1u)/(uint32_t)fbh;
		const size_t out_bytes = (size_t)bx*by*(size_t)bs;
		if (s.out_capacity < out_bytes)
			return fail(ctx, CFHIP_E_CAPACITY, "surface %zu: out_capacity %zu < %zu", i,
				s.out_capacity, out_bytes);
		if (device_mem && is_std_format(params->format) &&
			((((uintptr_t)s.out) & 15u) || (((uintptr_t)s.pixels) & (pb - 1)) || (apitch & (pb - 1))))
			return fail(ctx, CFHIP_E_INVALID, "surface %zu: standard formats need a 16-byte aligned "
				"device output and pixel-aligned source rows", i);
		if (items)
			items[i] = {row_bytes*(size_t)s.height, out_bytes, row_bytes};
	}
	return CFHIP_OK;
}

// `consumed(user, i)`: called once the library has finished READING surfaces[i].pixels (host path only): the
// caller may release that source then, as Converter::convert frees every source image as soon as its surface
// is converted (Converter.cpp:586) instead of holding the whole texture until the call returns.
static int encode_body(cfhip_ctx* ctx, StagingLease& lease, const cfhip_surface* surfaces, size_t n,
	const cfhip_params* params, bool device_mem, bool user_stream, cfhip_consumed_fn consumed, void* user);

// Every encode entry point of the C ABI comes through here.  The lease ends inside the frame: as an exception unwinds
// through it -- before guarded() turns that into an error code, and under the lock -- it drains whatever the body left
// queued on the staging buffers, as it does on an error return.
static int encode_impl(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n,
	const cfhip_params* params, bool device_mem, hipStream_t user_stream,
	cfhip_consumed_fn consumed = nullptr, void* user = nullptr)
{
	return guarded(ctx, "encode", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		StagingLease lease(ctx, user_stream ? user_stream : ctx->stream);
		return encode_body(ctx, lease, surfaces, n, params, device_mem, user_stream != nullptr, consumed, user);
	});
}

static int encode_body(cfhip_ctx* ctx, StagingLease& lease, const cfhip_surface* surfaces, size_t n,
	const cfhip_params* params, bool device_mem, bool user_stream, cfhip_consumed_fn consumed, void* user)
{
	int rc = check_params(ctx, params);
	if (rc != CFHIP_OK)
		return rc;
	if (!surfaces && n)
		return fail(ctx, CFHIP_E_INVALID, "surfaces is NULL");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const hipStream_t stream = lease.stream;
	begin_call(ctx, stream, nullptr);             // launch() names the kernel

	// validate everything first, compute sizes
	std::vector<Item> items(n);
	rc = validate_surfaces(ctx, surfaces, n, params, device_mem, items.data());
	if (rc != CFHIP_OK)
		return rc;
	int fbw, fbh;
	block_dims(params->format, &fbw, &fbh);

	if (device_mem) {
		size_t i0 = 0;
		while (i0 < n) {
			std::vector<cf_kparams> kps;
			size_t i1 = i0;
			while (i1 < n && surfaces[i1].pixel_type == surfaces[i0].pixel_type && kps.size() < 65536) {
				const cfhip_surface& s = surfaces[i1];
				cf_kparams kp;
				fill_kparams(kp, *params, s.pixels, s.out, (long long)s.row_pitch_bytes, s.width,
					s.height);
				kps.push_back(kp);
				++i1;
			}
			rc = batched_launch(ctx, lease, kps, *params, surfaces[i0].pixel_type);
			if (rc != CFHIP_OK)
				return rc;
			i0 = i1;
		}
	} else {
		// Host surfaces are processed in groups: every surface of a group is uploaded into
		// one staging buffer, all kernels are enqueued, all payloads downloaded, and the
		// stream is synchronised ONCE per group (Converter::convert instead joins its worker
		// threads once per surface, Converter.cpp:580-583 -- ruinous for mip tails).
		const size_t kGroupBytes = (size_t)512 << 20;
		// The strip pipeline pays where the host has work of its own to overlap: float sources of
		// 8-bit formats (quantised by host threads, 4x less PCIe traffic) and bottom-up images
		// (row gather).  A plain RGBA8 upload is faster as one pageable copy (measured: 9.3 vs
		// 9.9 ms for 4096x4096), and mid-size surfaces are better off batched in one launch.
		const size_t kPipelineBytes = (size_t)4 << 20;
		auto pipelined = [&](size_t i) {
			return surfaces[i].row_pitch_bytes < 0 ||
				(surfaces[i].pixel_type == CFHIP_PIXEL_RGBA32F && takes_unorm8(*params) &&
				 items[i].src_bytes >= kPipelineBytes);
		};
		size_t g0 = 0;
		while (g0 < n) {
			if (pipelined(g0)) {
				rc = encode_strip_pipeline(ctx, lease, surfaces[g0], *params);
				if (rc != CFHIP_OK)
					return rc;
				if (consumed)
					consumed(user, g0);
				++g0;
				continue;
			}
			size_t g1 = g0, src_total = 0, out_total = 0;
			while (g1 < n && (g1 == g0 || src_total + items[g1].src_bytes <= kGroupBytes) &&
				!pipelined(g1)) {
				src_total += (items[g1].src_bytes + 255) & ~(size_t)255;
				out_total += (items[g1].out_bytes + 255) & ~(size_t)255;
				++g1;
			}
			rc = lease.acquire();
			if (rc != CFHIP_OK) return rc;
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, src_total);
			if (rc != CFHIP_OK) return rc;
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, out_total);
			if (rc != CFHIP_OK) return rc;
			size_t so = 0, oo = 0;
			std::vector<size_t> out_off(g1 - g0);
			std::vector<cf_kparams> kps;
			int run_type = surfaces[g0].pixel_type;
			for (size_t i = g0; i < g1; ++i) {
				const cfhip_surface& s = surfaces[i];
				uint8_t* dsrc = static_cast<uint8_t*>(ctx->d_src) + so;
				uint8_t* dout = static_cast<uint8_t*>(ctx->d_out) + oo;
				if ((size_t)s.row_pitch_bytes == items[i].row_bytes)
					HIP_TRY(ctx, hipMemcpyAsync(dsrc, s.pixels, items[i].src_bytes,
						hipMemcpyHostToDevice, stream));
				else
					HIP_TRY(ctx, hipMemcpy2DAsync(dsrc, items[i].row_bytes, s.pixels,
						(size_t)s.row_pitch_bytes, items[i].row_bytes, s.height, hipMemcpyHostToDevice,
						stream));
				if (s.pixel_type != run_type && !kps.empty()) {
					rc = batched_launch(ctx, lease, kps, *params, run_type);
					if (rc != CFHIP_OK)
						return rc;
					kps.clear();
				}
				run_type = s.pixel_type;
				cf_kparams kp;
				fill_kparams(kp, *params, dsrc, dout, (long long)items[i].row_bytes, s.width, s.height);
				kps.push_back(kp);
				out_off[i - g0] = oo;
				so += (items[i].src_bytes + 255) & ~(size_t)255;
				oo += (items[i].out_bytes + 255) & ~(size_t)255;
			}
			// release hook: the sources are free once the group's uploads have left them -- an event behind the
			// last upload, waited for while the kernels run, not the end of the group's encode and download
			if (consumed) {
				if (!ctx->group_up)
					HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->group_up, hipEventDisableTiming));
				HIP_TRY(ctx, hipEventRecord(ctx->group_up, stream));
			}
			rc = batched_launch(ctx, lease, kps, *params, run_type);
			if (rc != CFHIP_OK)
				return rc;
			for (size_t i = g0; i < g1; ++i)
				HIP_TRY(ctx, hipMemcpyAsync(surfaces[i].out,
					static_cast<uint8_t*>(ctx->d_out) + out_off[i - g0], items[i].out_bytes,
					hipMemcpyDeviceToHost, stream));
			if (consumed) {
				HIP_TRY(ctx, hipEventSynchronize(ctx->group_up));
				for (size_t i = g0; i < g1; ++i)
					consumed(user, i);             // the group's uploads have left the host buffers
			}
			HIP_TRY(ctx, hipStreamSynchronize(stream));   // staging buffers are reused
			g0 = g1;
		}
	}
	return lease.done(!device_mem || !user_stream);
}

int cfhip_encode(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n_surfaces,
	const cfhip_params* params)
{
	return encode_impl(ctx, surfaces, n_surfaces, params, false, nullptr);
}

int cfhip_encode_multi(cfhip_ctx* const* ctxs, int n_ctx, const cfhip_surface* surfaces,
	size_t n_surfaces, const cfhip_params* params)
{
	return cfhip_encode_multi_ex(ctxs, n_ctx, surfaces, n_surfaces, params, nullptr, nullptr);
}

static int encode_multi_body(cfhip_ctx* const* ctxs, int n_ctx, const cfhip_surface* surfaces,
	size_t n_surfaces, const cfhip_params* params, cfhip_consumed_fn consumed, void* user);

int cfhip_encode_multi_ex(cfhip_ctx* const* ctxs, int n_ctx, const cfhip_surface* surfaces,
	size_t n_surfaces, const cfhip_params* params, cfhip_consumed_fn consumed, void* user)
{
	if (!ctxs || n_ctx <= 0 || !ctxs[0])
		return CFHIP_E_INVALID;
	// (the planning below builds vectors: an allocation failure there is an error code, not an exception across the C
	// ABI.  No lock here: the per-context encodes take each context's own in encode_impl, the first context's among
	// them, and a thread that cannot be started runs its share here)
	return no_throw(ctxs[0], "encode_multi", [&]() -> int {
		return encode_multi_body(ctxs, n_ctx, surfaces, n_surfaces, params, consumed, user);
	});
}

static int encode_multi_body(cfhip_ctx* const* ctxs, int n_ctx, const cfhip_surface* surfaces,
	size_t n_surfaces, const cfhip_params* params, cfhip_consumed_fn consumed, void* user)
{
	if (n_ctx == 1 || n_surfaces == 0)
		return encode_impl(ctxs[0], surfaces, n_surfaces, params, false, nullptr, consumed, user);
	if (!surfaces || !params)
		return fail(ctxs[0], CFHIP_E_INVALID, "null surfaces or params");
	for (int i = 0; i < n_ctx; ++i)
		if (!ctxs[i])
			return fail(ctxs[0], CFHIP_E_INVALID, "null context %d", i);
	int bw = 4, bh = 4, bs = 16;
	if (cfhip_query(params->format, params->type, &bw, &bh, &bs) != CFHIP_OK)
		return fail(ctxs[0], CFHIP_E_UNSUPPORTED, "format %d with type %d is not supported", params->format, params->type);
	if (consumed) {
		// with a release hook nothing may be read before everything that can be checked has been
		int vrc = check_params(ctxs[0], params);
		if (vrc == CFHIP_OK)
			vrc = validate_surfaces(ctxs[0], surfaces, n_surfaces, params, false, nullptr);
		if (vrc != CFHIP_OK)
			return vrc;
	}
	// Work units.  The reference parallelises WITHIN a surface (jobsX*jobsY jobs on an atomic
	// counter, Converter.cpp:540-583) as well as over nothing else, so one big surface must not pin
	// the call to one GPU: a surface holding more than 1/n_ctx of the call's blocks is cut into
	// n_ctx ranges of whole block rows (cfhip_shard_rows).  A range is a
	// surface of its own -- `pixels` advanced by whole block rows, `out` by the rows' payload --
	// and only the last range sees the true bottom edge, so edge replication and the ETC border
	// rule act exactly as in the unsplit surface: same bytes.
	std::vector<uint64_t> sblocks(n_surfaces);
	uint64_t total = 0;
	for (size_t i = 0; i < n_surfaces; ++i) {
		sblocks[i] = (uint64_t)((surfaces[i].width + (uint32_t)bw - 1u)/(uint32_t)bw)*
			((surfaces[i].height + (uint32_t)bh - 1u)/(uint32_t)bh);
		total += sblocks[i];
	}
	// rows of a standard format are cut in multiples of 4 so that every range's payload keeps the
	// 4-byte alignment the packers store with
	const uint32_t row_quant = is_std_format(params->format) ? 4u : 1u;
	// below this a second launch (host thread, upload, launch, synchronisation) costs more than it saves: 4 096
	// blocks of a block format = 65 536 texels; a standard format's "block" is ONE pixel, so the same area there
	const uint64_t kMinSplitBlocks = is_std_format(params->format) ? 65536 : 4096;
	std::vector<cfhip_surface> units;
	std::vector<uint64_t> blocks;
	std::vector<size_t> origin;           // the surface a unit was cut from
	units.reserve(n_surfaces + (size_t)n_ctx);
	for (size_t i = 0; i < n_surfaces; ++i) {
		const cfhip_surface& s = surfaces[i];
		const uint32_t bx = (s.width + (uint32_t)bw - 1u)/(uint32_t)bw;
		const uint32_t by = (s.height + (uint32_t)bh - 1u)/(uint32_t)bh;
		const bool split = sblocks[i]*(uint64_t)n_ctx > total && sblocks[i] >= kMinSplitBlocks &&
			by/row_quant >= 2u && s.pixels && s.out && s.pixel_type >= CFHIP_PIXEL_RGBA8 &&
			s.pixel_type <= CFHIP_PIXEL_RGBA16F;
		if (!split) {
			units.push_back(s);
			blocks.push_back(sblocks[i]);
			origin.push_back(i);
			continue;
		}
		const uint32_t qrows = (by + row_quant - 1u)/row_quant;     // rows in units of row_quant
		const int parts = (int)std::min<uint32_t>((uint32_t)n_ctx, qrows);
		for (int r = 0; r < parts; ++r) {
			uint32_t q0, q1;
			cfhip_shard_rows(qrows, r, parts, &q0, &q1);
			const uint32_t br0 = q0*row_quant, br1 = std::min(by, q1*row_quant);
			if (br1 <= br0)
				continue;
			const uint32_t y0 = br0*(uint32_t)bh, y1 = std::min(s.height, br1*(uint32_t)bh);
			cfhip_surface u = s;
			u.pixels = static_cast<const uint8_t*>(s.pixels) + (ptrdiff_t)y0*s.row_pitch_bytes;
			u.height = y1 - y0;
			const size_t off = (size_t)br0*bx*(size_t)bs;
			u.out = static_cast<uint8_t*>(s.out) + off;
			// the capacity check of the whole surface is kept: a range may use what is left of it
			u.out_capacity = s.out_capacity > off ? s.out_capacity - off : 0;
			if (r + 1 < parts)
				u.out_capacity = std::min(u.out_capacity, (size_t)(br1 - br0)*bx*(size_t)bs);
			units.push_back(u);
			blocks.push_back((uint64_t)(br1 - br0)*bx);
			origin.push_back(i);
		}
	}
	const size_t n_units = units.size();
	// longest-processing-time assignment on block counts: units by (blocks desc, index asc),
	// each to the least loaded context (ties: the lowest index) -- cuttlefish_amd/shard.py's rule
	std::vector<size_t> order(n_units);
	for (size_t i = 0; i < n_units; ++i)
		order[i] = i;
	std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return blocks[a] > blocks[b]; });
	std::vector<std::vector<cfhip_surface>> share((size_t)n_ctx);
	std::vector<std::vector<size_t>> share_origin((size_t)n_ctx);
	std::vector<uint64_t> load((size_t)n_ctx, 0);
	for (size_t i : order) {
		size_t k = 0;
		for (size_t c = 1; c < (size_t)n_ctx; ++c)
			if (load[c] < load[k])
				k = c;
		share[k].push_back(units[i]);
		share_origin[k].push_back(origin[i]);
		load[k] += blocks[i];
	}
	// a surface is consumed when the last of its units is: one counter per surface, the contexts' threads
	// report their units through it (the caller's function may therefore run on any of them, for different
	// surfaces at the same time)
	std::vector<std::atomic<int>> pending(consumed ? n_surfaces : 0);
	if (consumed)
		for (size_t u = 0; u < n_units; ++u)
			pending[origin[u]].fetch_add(1, std::memory_order_relaxed);
	struct Relay { cfhip_consumed_fn fn; void* user; const std::vector<size_t>* origin; std::vector<std::atomic<int>>* pending; };
	std::vector<Relay> relay((size_t)n_ctx);
	for (int c = 0; c < n_ctx; ++c)
		relay[(size_t)c] = {consumed, user, &share_origin[(size_t)c], &pending};
	const cfhip_consumed_fn unit_done = [](void* r_, size_t unit) {
		Relay* r = static_cast<Relay*>(r_);
		const size_t surf = (*r->origin)[unit];
		if ((*r->pending)[surf].fetch_sub(1, std::memory_order_acq_rel) == 1)
			r->fn(r->user, surf);
	};
	std::vector<int> rc((size_t)n_ctx, CFHIP_OK);
	std::vector<std::thread> workers;
	std::vector<char> started((size_t)n_ctx, 0);
	workers.reserve((size_t)n_ctx);
	for (int c = 1; c < n_ctx; ++c)
		if (!share[(size_t)c].empty()) {
			try {
				workers.emplace_back([&, c]() {
					rc[(size_t)c] = encode_impl(ctxs[c], share[(size_t)c].data(), share[(size_t)c].size(), params, false, nullptr,
						consumed ? unit_done : nullptr, &relay[(size_t)c]);
				});
				started[(size_t)c] = 1;
			} catch (...) {
				// no thread to be had (pids limit): this context's share runs on the calling thread, below
			}
		}
	for (int c = 0; c < n_ctx; ++c)
		if (!share[(size_t)c].empty() && !started[(size_t)c])
			rc[(size_t)c] = encode_impl(ctxs[c], share[(size_t)c].data(), share[(size_t)c].size(), params, false, nullptr,
				consumed ? unit_done : nullptr, &relay[(size_t)c]);
	for (std::thread& t : workers)
		t.join();
	for (int c = 0; c < n_ctx; ++c)
		if (rc[(size_t)c] != CFHIP_OK)
			return rc[(size_t)c];
	return CFHIP_OK;
}

int cfhip_encode_device(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n_surfaces,
	const cfhip_params* params, void* stream)
{
	return encode_impl(ctx, surfaces, n_surfaces, params, true, static_cast<hipStream_t>(stream));
}

// Image::ResizeFilter 0..4, Box / Linear optionally with the fallback flag
static bool filter_valid(int filter)
{
	const int base = filter & ~CFHIP_FILTER_FALLBACK;
	if (base < CFHIP_FILTER_BOX || base > CFHIP_FILTER_BSPLINE)
		return false;
	return !(filter & CFHIP_FILTER_FALLBACK) || base <= CFHIP_FILTER_LINEAR;
}

// The argument checks every mip / resize entry point shares, in this order; `what` names the entry point in the
// messages.  depth 0: a 2-D texture.
static int check_mip_args(cfhip_ctx* ctx, const char* what, int pixel_type, int color_space, int filter,
	uint32_t width, uint32_t height, uint32_t depth, uint32_t levels, size_t pitch)
{
	if (pixel_type < CFHIP_PIXEL_RGBA8 || pixel_type > CFHIP_PIXEL_RGBA16F)
		return fail(ctx, CFHIP_E_INVALID, "%s: pixel type %d", what, pixel_type);
	if (color_space != CFHIP_COLOR_LINEAR && color_space != CFHIP_COLOR_SRGB)
		return fail(ctx, CFHIP_E_INVALID, "%s: colour space %d", what, color_space);
	if (!filter_valid(filter))
		return fail(ctx, CFHIP_E_INVALID, "%s: resize filter %d", what, filter);
	// maxMipmapLevels: floor(log2(max(w, h, d))) + 1 (Texture.cpp)
	const uint32_t max_levels = chain_levels(std::max(width, depth), height);
	if (levels > max_levels && depth)
		return fail(ctx, CFHIP_E_INVALID, "%u mip levels requested, a %ux%ux%u texture has %u", levels,
			width, height, depth, max_levels);
	if (levels > max_levels)
		return fail(ctx, CFHIP_E_INVALID, "%u mip levels requested, a %ux%u texture has %u", levels,
			width, height, max_levels);
	if (pitch < (size_t)width*pixel_bytes(pixel_type))
		return fail(ctx, CFHIP_E_INVALID, "%s: row pitch smaller than a row", what);
	return CFHIP_OK;
}

// One 2-D resize of Image::resize (Image.cpp:1324-1511): prev (any pixel type) -> dst (RGBA32F,
// tightly packed w x h): FreeImage_Rescale's two passes for all five filters; one kernel for the
// in-tree fallback of Box / Linear (CFHIP_FILTER_FALLBACK).
static int mip_level_2d(cfhip_ctx* ctx, StagingLease& lease, const void* prev, int prev_type, size_t prev_pitch,
	uint32_t pw, uint32_t ph, void* dst, uint32_t w, uint32_t h, int filter, int srgb)
{
	const hipStream_t stream = lease.stream;
	if (filter & CFHIP_FILTER_FALLBACK) {
		// the loops Image::resize runs itself when FreeImage_Rescale fails (Image.cpp:1393-1505)
		HIP_TRY(ctx, cfhip_launch_mip_resize(prev, prev_type, prev_pitch, pw, ph, dst, w, h, filter & 0xFF, srgb,
			stream));
		return CFHIP_OK;
	}
	// FreeImage_Rescale's two passes, horizontal first when dst_w*src_h <= dst_h*src_w, with a
	// float intermediate image in the context's staging buffer; a pass whose size does
	// not change is skipped (the other one then does both colour conversions)
	const bool x_first = (unsigned long long)w*ph <= (unsigned long long)h*pw;
	const bool need_x = w != pw, need_y = h != ph;
	// the fused kernel does taps_x * taps_y work per output texel: it beats the two passes (24 -> 8 bytes per
	// texel) only while the footprint is small -- a mip step (2:1, at most 3 x 3 taps with an odd size).  A
	// resize of a custom mip image can have any ratio (1024 x 1024 -> 1 x 1: a million taps in one thread
	// against 2 x 1024 for the separable passes): those take the two-pass route
	const bool small_taps = (unsigned long long)pw <= 2ull*w + 1ull && (unsigned long long)ph <= 2ull*h + 1ull;
	if (need_x && need_y && filter == CFHIP_FILTER_BOX && small_taps) {
		// the box filter: both passes in one launch, no float image in between (bit-identical)
		HIP_TRY(ctx, cfhip_launch_mip_fused_layers(prev, prev_type, prev_pitch, pw, ph, dst, w, h,
			x_first ? 1 : 0, filter, srgb, 1u, nullptr, nullptr, 0, 0, stream));
	} else if (need_x && need_y) {
		const uint32_t tw = x_first ? w : pw, th = x_first ? ph : h;
		int rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, (size_t)tw*th*16u);
		if (rc != CFHIP_OK)
			return rc;
		HIP_TRY(ctx, cfhip_launch_mip_pass(prev, prev_type, prev_pitch, x_first ? pw : ph, ctx->d_src, tw, th,
			x_first ? 1 : 0, filter, srgb, 0, stream));
		HIP_TRY(ctx, cfhip_launch_mip_pass(ctx->d_src, CFHIP_PIXEL_RGBA32F, (size_t)tw*16u, x_first ? ph : pw,
			dst, w, h, x_first ? 0 : 1, filter, 0, srgb, stream));
	} else {
		HIP_TRY(ctx, cfhip_launch_mip_pass(prev, prev_type, prev_pitch, need_x ? pw : ph, dst, w, h,
			need_x ? 1 : 0, filter, srgb, srgb, stream));
	}
	return CFHIP_OK;
}

int cfhip_generate_mips_device(cfhip_ctx* ctx, const void* src, int src_pixel_type,
	uint32_t width, uint32_t height, size_t src_pitch_bytes, int color_space, int filter,
	void* const* dst_levels, uint32_t levels, void* stream_)
{
	return guarded(ctx, "mip generation", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		if (!src || !width || !height || !levels || (levels > 1 && !dst_levels))
			return fail(ctx, CFHIP_E_INVALID, "mip generation: NULL or empty argument");
		int rc = check_mip_args(ctx, "mip generation", src_pixel_type, color_space, filter, width, height, 0, levels,
			src_pitch_bytes);
		if (rc != CFHIP_OK)
			return rc;
		for (uint32_t k = 1; k < levels; ++k)
			if (!dst_levels[k - 1])
				return fail(ctx, CFHIP_E_INVALID, "mip generation: dst_levels[%u] is NULL", k - 1);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		// (no begin_call: the launches of mip generation and resize are untimed and leave last_kernel alone)
		StagingLease lease(ctx, call_stream(ctx, stream_));
		// level k from level k-1, as Texture::generateMipmaps does (Texture.cpp:1480-1487)
		const void* prev = src;
		int prev_type = src_pixel_type;
		size_t prev_pitch = src_pitch_bytes;
		uint32_t pw = width, ph = height;
		for (uint32_t k = 1; k < levels; ++k) {
			const uint32_t w = (width >> k) ? (width >> k) : 1u, h = (height >> k) ? (height >> k) : 1u;
			rc = mip_level_2d(ctx, lease, prev, prev_type, prev_pitch, pw, ph, dst_levels[k - 1], w, h, filter,
				color_space == CFHIP_COLOR_SRGB ? 1 : 0);
			if (rc != CFHIP_OK)
				return rc;
			prev = dst_levels[k - 1];
			prev_type = CFHIP_PIXEL_RGBA32F;
			prev_pitch = (size_t)w*16u;
			pw = w; ph = h;
		}
		return lease.done(!stream_);
	});
}

// Array / cube textures: Texture::generateMipmaps resizes every [depth][face] image of a level on its own
// (Texture.cpp:1480-1511 inside its loops over depth and faces) -- the layers never mix.  Here the layers
// of a level share ONE launch per pass (blockIdx.z = layer): a 2048^2 chain is 22 launches of which 16
// are a few microseconds long, and an array of 256 such textures was 5 632 dependent launches on one
// stream (launch-bound: 28 ms); batched it is 22.  A level whose staging image for all layers would
// pass the budget below runs layer by layer -- those launches are long enough not to matter.
int cfhip_generate_mips_array_device(cfhip_ctx* ctx, const void* const* srcs, uint32_t layers,
	int src_pixel_type, uint32_t width, uint32_t height, size_t src_pitch_bytes, int color_space,
	int filter, void* const* dst_levels, uint32_t levels, void* stream_)
{
	return guarded(ctx, "mip generation", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		if (!srcs || !layers || !width || !height || !levels || (levels > 1 && !dst_levels))
			return fail(ctx, CFHIP_E_INVALID, "mip generation: NULL or empty argument");
		if (layers > 65535u)
			return fail(ctx, CFHIP_E_INVALID, "mip generation: %u layers (at most 65535 per call)", layers);
		int rc = check_mip_args(ctx, "mip generation", src_pixel_type, color_space, filter, width, height, 0, levels,
			src_pitch_bytes);
		if (rc != CFHIP_OK)
			return rc;
		for (uint32_t l = 0; l < layers; ++l) {
			if (!srcs[l])
				return fail(ctx, CFHIP_E_INVALID, "mip generation: srcs[%u] is NULL", l);
			for (uint32_t k = 1; k < levels; ++k)
				if (!dst_levels[(size_t)l*(levels - 1u) + (k - 1u)])
					return fail(ctx, CFHIP_E_INVALID, "mip generation: dst_levels[%u][%u] is NULL", l, k - 1u);
		}
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		const hipStream_t stream = lease.stream;
		const int srgb = color_space == CFHIP_COLOR_SRGB ? 1 : 0;
		if (levels > 1) {
			// device pointer tables, level-major: row 0 = the sources, row k = level k of every layer
			std::vector<const void*> tab((size_t)levels*layers);
			for (uint32_t l = 0; l < layers; ++l) {
				tab[l] = srcs[l];
				for (uint32_t k = 1; k < levels; ++k)
					tab[(size_t)k*layers + l] = dst_levels[(size_t)l*(levels - 1u) + (k - 1u)];
			}
			rc = lease.acquire();
			if (rc == CFHIP_OK)
				rc = reserve(ctx, &ctx->d_batch, &ctx->batch_cap, tab.size()*sizeof(void*));
			if (rc != CFHIP_OK)
				return rc;
			// pageable source: the runtime stages the copy before returning, so `tab` may die
			if (hipMemcpyAsync(ctx->d_batch, tab.data(), tab.size()*sizeof(void*), hipMemcpyHostToDevice, stream) != hipSuccess)
				return fail(ctx, CFHIP_E_DEVICE, "mip generation: table upload failed");
			const void* const* d_tab = static_cast<const void* const*>(ctx->d_batch);
			const size_t kStagingBudget = (size_t)1 << 30;           // the float image between the two passes, all layers
			uint32_t pw = width, ph = height;
			int prev_type = src_pixel_type;
			size_t prev_pitch = src_pitch_bytes;
			for (uint32_t k = 1; k < levels; ++k) {
				const uint32_t w = (width >> k) ? (width >> k) : 1u, h = (height >> k) ? (height >> k) : 1u;
				const void* const* s_tab = d_tab + (size_t)(k - 1u)*layers;
				void* const* o_tab = const_cast<void* const*>(d_tab + (size_t)k*layers);
				const bool x_first = (unsigned long long)w*ph <= (unsigned long long)h*pw;
				const bool need_x = w != pw, need_y = h != ph;
				const uint32_t tw = x_first ? w : pw, th = x_first ? ph : h;
				const size_t timg = (size_t)tw*th*16u;
				const bool fused = filter == CFHIP_FILTER_BOX && need_x && need_y;
				const bool batched = !(filter & CFHIP_FILTER_FALLBACK) && (fused || !(need_x && need_y) || timg*layers <= kStagingBudget);
				hipError_t e = hipSuccess;
				if (fused) {
					e = cfhip_launch_mip_fused_layers(nullptr, prev_type, prev_pitch, pw, ph, nullptr, w, h,
						x_first ? 1 : 0, filter, srgb, layers, s_tab, o_tab, 0, 0, stream);
				} else if (!batched) {
					for (uint32_t l = 0; l < layers; ++l) {
						rc = mip_level_2d(ctx, lease, tab[(size_t)(k - 1u)*layers + l], prev_type, prev_pitch, pw, ph,
							const_cast<void*>(tab[(size_t)k*layers + l]), w, h, filter, srgb);
						if (rc != CFHIP_OK)
							return rc;
					}
				} else if (need_x && need_y) {
					rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, timg*layers);
					if (rc != CFHIP_OK)
						return rc;
					e = cfhip_launch_mip_pass_layers(nullptr, prev_type, prev_pitch, x_first ? pw : ph, ctx->d_src, tw, th,
						x_first ? 1 : 0, filter, srgb, 0, layers, s_tab, nullptr, 0, timg, stream);
					if (e == hipSuccess)
						e = cfhip_launch_mip_pass_layers(ctx->d_src, CFHIP_PIXEL_RGBA32F, (size_t)tw*16u, x_first ? ph : pw, nullptr, w, h,
							x_first ? 0 : 1, filter, 0, srgb, layers, nullptr, o_tab, timg, 0, stream);
				} else {
					e = cfhip_launch_mip_pass_layers(nullptr, prev_type, prev_pitch, need_x ? pw : ph, nullptr, w, h,
						need_x ? 1 : 0, filter, srgb, srgb, layers, s_tab, o_tab, 0, 0, stream);
				}
				if (e != hipSuccess)
					return fail(ctx, CFHIP_E_DEVICE, "mip pass: %s", hipGetErrorString(e));
				prev_type = CFHIP_PIXEL_RGBA32F;
				prev_pitch = (size_t)w*16u;
				pw = w; ph = h;
			}
		}
		return lease.done(!stream_);
	});
}

// ---- mip post-pass (csrc/mip_post.hip): alpha-test coverage and normal renormalisation ---------------------------
// the alpha component must be loadable: its size divides the pointer and the pitch
static bool alpha_aligned(const void* p, size_t pitch, int pixel_type)
{
	const size_t a = pixel_type == CFHIP_PIXEL_RGBA8 ? 1u : pixel_type == CFHIP_PIXEL_RGBA16F ? 2u : 4u;
	return (uintptr_t)p % a == 0 && pitch % a == 0;
}

int cfhip_alpha_coverage_device(cfhip_ctx* ctx, const cfhip_coverage_surface* surfaces, uint32_t count, float threshold,
	float scale, uint32_t* counts_device, void* stream_)
{
	return guarded(ctx, "alpha_coverage", [&]() -> int {
		const char* const what = "alpha_coverage";
		CF_TRY(check_given(ctx, what, "surfaces", surfaces));
		CF_TRY(check_given(ctx, what, "counts_device", counts_device));
		if (!count)
			return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: count is 0");
		if (!(threshold > 0.0f && threshold <= 1.0f))
			return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: threshold %g outside (0, 1]", (double)threshold);
		if (!(scale > 0.0f) || std::isinf(scale))
			return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: scale %g is not a positive finite number", (double)scale);
		std::vector<cfmp_surf> tab(count);
		uint64_t wg = 0;
		for (uint32_t i = 0; i < count; ++i) {
			const cfhip_coverage_surface& s = surfaces[i];
			if (!s.pixels)
				return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: surfaces[%u].pixels is NULL", i);
			if (!s.width || !s.height)
				return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: surfaces[%u] has a zero width or height", i);
			const size_t pb = pixel_bytes(s.pixel_type);
			if (!pb)
				return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: surfaces[%u]: pixel type %d", i, s.pixel_type);
			if (s.pitch_bytes < (size_t)s.width*pb)
				return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: surfaces[%u]: pitch_bytes %zu < %zu", i, s.pitch_bytes,
					(size_t)s.width*pb);
			if ((uint64_t)s.width*s.height > CFMP_MAX_TEXELS)
				return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: surfaces[%u]: more than 2^30 texels", i);
			if (!alpha_aligned(s.pixels, s.pitch_bytes, s.pixel_type))
				return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: surfaces[%u]: pixels or pitch_bytes not aligned to a component", i);
			cfmp_surf& e = tab[i];
			e.pixels = static_cast<const uint8_t*>(s.pixels);
			e.pitch = s.pitch_bytes;
			e.plane_off = 0;
			e.width = s.width; e.height = s.height;
			e.n = s.width*s.height;
			e.pixel_type = s.pixel_type;
			e.wg_begin = (uint32_t)wg;
			e.ref = 0;
			wg += (e.n + CFMP_CHUNK - 1u)/CFMP_CHUNK;
			if (wg > 0x7FFFFFFFull)
				return fail(ctx, CFHIP_E_INVALID, "alpha_coverage: the surfaces are too large for one launch");
		}
		const size_t tab_bytes = tab.size()*sizeof(cfmp_surf);
		return device_pass(ctx, stream_, "cfhip_mip_post_gather_kernel", tab_bytes, 0, [&](hipStream_t stream) -> int {
			// pageable source: the runtime stages the copy before returning, so `tab` may die
			HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, tab.data(), tab_bytes, hipMemcpyHostToDevice, stream));
			HIP_TRY(ctx, hipMemsetAsync(counts_device, 0, (size_t)count*4u, stream));
			return timed(ctx, stream, "mip post-pass", [&] {
				return cfhip_launch_mip_post_gather(static_cast<const cfmp_surf*>(ctx->d_batch), count, 0u, (uint32_t)wg, threshold,
					scale, scale, scale, 1u, 1u, nullptr, counts_device, stream);
			});
		});
	});
}

int cfhip_mip_post_array_device(cfhip_ctx* ctx, const void* const* srcs, uint32_t layers, int src_pixel_type,
	uint32_t width, uint32_t height, size_t src_pitch_bytes, void* const* levels, uint32_t levels_count,
	const cfhip_mip_post_params* params, cfhip_mip_post_result* results_device, void* stream_)
{
	static_assert(sizeof(cfhip_mip_post_params) == 8 && sizeof(cfhip_mip_post_result) == 16, "the ABI's sizes");
	return guarded(ctx, "mip_post", [&]() -> int {
		const char* const what = "mip_post";
		CF_TRY(check_given(ctx, what, "params", params));
		CF_TRY(check_given(ctx, what, "srcs", srcs));
		CF_TRY(check_given(ctx, what, "levels", levels));
		CF_TRY(check_layers(ctx, what, layers));
		if (!width || !height)
			return fail(ctx, CFHIP_E_INVALID, "mip_post: a zero width or height (%ux%u)", width, height);
		size_t pb;
		CF_TRY(check_pixel_type(ctx, what, "src_pixel_type", src_pixel_type, &pb));
		const uint32_t max_levels = chain_levels(width, height);
		if (levels_count < 2 || levels_count > max_levels)
			return fail(ctx, CFHIP_E_INVALID, "mip_post: levels_count is %u, a chain to repair has 2 to %u levels at %ux%u",
				levels_count, max_levels, width, height);
		const uint32_t flags = params->flags;
		const uint32_t all_flags = CFHIP_MIP_POST_COVERAGE | CFHIP_MIP_POST_NORMALIZE | CFHIP_MIP_POST_SIGNED_NORMALS;
		if (!flags || (flags & ~all_flags))
			return fail(ctx, CFHIP_E_INVALID, "mip_post: params->flags 0x%x: none or unknown", flags);
		if ((flags & CFHIP_MIP_POST_SIGNED_NORMALS) && !(flags & CFHIP_MIP_POST_NORMALIZE))
			return fail(ctx, CFHIP_E_INVALID, "mip_post: params->flags: SIGNED_NORMALS without NORMALIZE");
		const bool coverage = flags & CFHIP_MIP_POST_COVERAGE;
		const float t = params->alpha_threshold;
		if (coverage && !(t > 0.0f && t <= 1.0f))
			return fail(ctx, CFHIP_E_INVALID, "mip_post: params->alpha_threshold %g outside (0, 1]", (double)t);
		CF_TRY(check_row_pitch(ctx, what, "src_pitch_bytes", src_pitch_bytes, (size_t)width*pb));
		if (coverage && !results_device)
			return fail(ctx, CFHIP_E_INVALID, "mip_post: results_device is NULL under COVERAGE");
		if ((uint64_t)width*height > CFMP_MAX_TEXELS)
			return fail(ctx, CFHIP_E_INVALID, "mip_post: more than 2^30 texels in level 0");
		const uint32_t per = levels_count - 1u;
		const size_t nlev = (size_t)layers*per, nsurf = nlev + (coverage ? layers : 0u);
		std::vector<cfmp_surf> tab(nsurf);
		uint64_t wg = 0, plane = 0;
		for (uint32_t l = 0; l < layers; ++l) {
			CF_TRY(check_item_given(ctx, what, "srcs", l, srcs[l]));
			if (coverage && !alpha_aligned(srcs[l], src_pitch_bytes, src_pixel_type))
				return fail(ctx, CFHIP_E_INVALID, "mip_post: srcs[%u] or src_pitch_bytes not aligned to a component", l);
			for (uint32_t k = 1; k < levels_count; ++k) {
				CF_TRY(check_chain_level(ctx, what, levels, per, l, k));
				const size_t i = (size_t)l*per + (k - 1u);
				cfmp_surf& e = tab[i];
				e.width = (width >> k) ? (width >> k) : 1u;
				e.height = (height >> k) ? (height >> k) : 1u;
				e.pixels = static_cast<const uint8_t*>(levels[i]);
				e.pitch = (unsigned long long)e.width*16u;
				e.plane_off = plane;
				e.n = e.width*e.height;
				e.pixel_type = CFHIP_PIXEL_RGBA32F;
				e.wg_begin = (uint32_t)wg;
				e.ref = (uint32_t)(nlev + l);
				wg += (e.n + CFMP_CHUNK - 1u)/CFMP_CHUNK;
				plane += e.n;
			}
		}
		const uint64_t wg_levels = wg;
		for (uint32_t l = 0; coverage && l < layers; ++l) {
			cfmp_surf& e = tab[nlev + l];
			e.pixels = static_cast<const uint8_t*>(srcs[l]);
			e.pitch = src_pitch_bytes;
			e.plane_off = 0;
			e.width = width; e.height = height;
			e.n = width*height;
			e.pixel_type = src_pixel_type;
			e.wg_begin = (uint32_t)wg;
			e.ref = 0;
			wg += (e.n + CFMP_CHUNK - 1u)/CFMP_CHUNK;
		}
		if (wg > 0x7FFFFFFFull)
			return fail(ctx, CFHIP_E_INVALID, "mip_post: the surfaces are too large for one launch");
		// d_batch: the surface table, then the levels' search states, then the counters; d_src: the alpha plane
		const size_t tab_bytes = (nsurf*sizeof(cfmp_surf) + 15u) & ~(size_t)15u;
		const size_t state_bytes = coverage ? nlev*sizeof(cfmp_state) : 0u;
		const size_t cnt_bytes = coverage ? nsurf*CFMP_SLOTS*4u : 0u;
		const char* const kernel = coverage ? "cfhip_mip_post_count_kernel" : "cfhip_mip_post_apply_kernel";
		return device_pass(ctx, stream_, kernel, tab_bytes + state_bytes + cnt_bytes, coverage ? (size_t)plane*4u : 0u,
			[&](hipStream_t stream) -> int {
			uint8_t* base = static_cast<uint8_t*>(ctx->d_batch);
			const cfmp_surf* d_tab = reinterpret_cast<const cfmp_surf*>(base);
			cfmp_state* d_state = coverage ? reinterpret_cast<cfmp_state*>(base + tab_bytes) : nullptr;
			uint32_t* d_cnt = reinterpret_cast<uint32_t*>(base + tab_bytes + state_bytes);
			// pageable source: the runtime stages the copy before returning, so `tab` may die
			HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, tab.data(), nsurf*sizeof(cfmp_surf), hipMemcpyHostToDevice, stream));
			LaunchChain post(ctx, stream, "mip post-pass");
			if (coverage) {
				// (the states too: a level's first decide step writes every field it later reads, dir included)
				HIP_TRY(ctx, hipMemsetAsync(base + tab_bytes, 0, state_bytes + cnt_bytes, stream));
				float* d_plane = static_cast<float*>(ctx->d_src);
				const float s_min = 0.25f, s_max = 4.0f;
				const auto decide = [&](int first) {
					post([&] {
						return cfhip_launch_mip_post_decide(d_tab, (uint32_t)nlev, first, d_state, d_cnt, results_device, stream);
					});
				};
				post([&] {
					return cfhip_launch_mip_post_gather(d_tab, (uint32_t)nsurf, (uint32_t)nlev, (uint32_t)wg, t, 1.0f, s_min, s_max, 3u,
						CFMP_SLOTS, d_plane, d_cnt, stream);
				});
				decide(1);
				for (uint32_t pass = 0; pass < CFMP_SEARCH_PASSES; ++pass) {
					post([&] {
						return cfhip_launch_mip_post_count(d_tab, (uint32_t)nlev, (uint32_t)wg_levels, t, d_state, d_plane, d_cnt, stream);
					});
					decide(0);
				}
			}
			post([&] {
				return cfhip_launch_mip_post_apply(d_tab, (uint32_t)nlev, (uint32_t)wg_levels, flags, d_state, stream);
			});
			return post.rc;
		});
	});
}

// ---- alpha bleeding (csrc/alpha_bleed.hip): colour under transparent texels from the nearest visible one -------------
int cfhip_alpha_bleed_array_device(cfhip_ctx* ctx, void* const* images, uint32_t layers, int pixel_type, uint32_t width,
	uint32_t height, size_t pitch_bytes, const cfhip_bleed_params* params, cfhip_bleed_result* results_device, void* stream_)
{
	static_assert(sizeof(cfhip_bleed_params) == 12 && sizeof(cfhip_bleed_result) == 16, "the ABI's sizes");
	return guarded(ctx, "alpha_bleed", [&]() -> int {
		const char* const what = "alpha_bleed";
		CF_TRY(check_given(ctx, what, "params", params));
		CF_TRY(check_given(ctx, what, "images", images));
		CF_TRY(check_layers(ctx, what, layers));
		CF_TRY(check_sides(ctx, what, width, height, CFAB_MAX_SIDE));
		size_t pb;
		CF_TRY(check_pixel_type(ctx, what, "pixel_type", pixel_type, &pb));
		CF_TRY(check_flags(ctx, what, params->flags, CFHIP_BLEED_WRAP_X | CFHIP_BLEED_WRAP_Y));
		const float t = params->alpha_threshold;
		CF_TRY(check_threshold(ctx, what, t));
		if (params->max_distance > 65535u)
			return fail(ctx, CFHIP_E_INVALID, "alpha_bleed: params->max_distance %u above 65535", params->max_distance);
		CF_TRY(check_row_pitch(ctx, what, "pitch_bytes", pitch_bytes, (size_t)width*pb));
		CF_TRY(check_pitch_aligned(ctx, what, "pitch_bytes", pitch_bytes, pb/4u, "a component"));
		const uint64_t texels = (uint64_t)layers*width*height;
		if (texels > CFAB_MAX_TEXELS)
			return fail(ctx, CFHIP_E_INVALID, "alpha_bleed: more than 2^31 texels in one call");
		for (uint32_t l = 0; l < layers; ++l) {
			CF_TRY(check_item_given(ctx, what, "images", l, images[l]));
			CF_TRY(check_item_aligned(ctx, what, "images", l, images[l], pb/4u, "a component"));
		}
		// d_batch: the layers' pointers; d_src: the two seed buffers, 4 bytes per texel each
		return device_pass(ctx, stream_, "cfhip_alpha_bleed_step_kernel", (size_t)layers*sizeof(void*), (size_t)texels*8u,
			[&](hipStream_t stream) -> int {
			void** table[1];
			CF_TRY(upload_tables(ctx, stream, {{images, layers}}, table));
			if (results_device)
				HIP_TRY(ctx, hipMemsetAsync(results_device, 0, (size_t)layers*sizeof(cfhip_bleed_result), stream));
			cfab_call call;
			call.images = table[0];
			call.pitch = pitch_bytes;
			call.width = width; call.height = height;
			call.pixel_type = pixel_type;
			call.flags = params->flags;
			uint32_t* buf[2] = {static_cast<uint32_t*>(ctx->d_src), static_cast<uint32_t*>(ctx->d_src) + texels};
			uint32_t p2 = 1;
			while (p2 < std::max(width, height))
				p2 <<= 1;
			// on a wrapped axis positions are taken modulo the size: so is the step
			const auto sx = [&](uint32_t k) { return (call.flags & CFHIP_BLEED_WRAP_X) ? k % width : k; };
			const auto sy = [&](uint32_t k) { return (call.flags & CFHIP_BLEED_WRAP_Y) ? k % height : k; };
			LaunchChain bleed(ctx, stream, "alpha_bleed");
			bleed([&] { return cfhip_launch_alpha_bleed_seed(&call, layers, t, buf[0], results_device, stream); });
			int cur = 0;
			for (uint32_t k = p2 >> 1; k >= 1u; k >>= 1, cur ^= 1)
				bleed([&] { return cfhip_launch_alpha_bleed_step(&call, layers, sx(k), sy(k), buf[cur], buf[cur ^ 1], stream); });
			bleed([&] {
				return cfhip_launch_alpha_bleed_fill(&call, layers, sx(1u), sy(1u), params->max_distance*params->max_distance,
					buf[cur], results_device, stream);
			});
			return bleed.rc;
		});
	});
}

// ---- signed distance field from alpha (csrc/alpha_sdf.hip): exact to the spread, 0.5 at the silhouette --------------
int cfhip_alpha_sdf_array_device(cfhip_ctx* ctx, const void* const* src, uint32_t layers, int src_pixel_type, uint32_t width,
	uint32_t height, size_t src_pitch_bytes, void* const* dst, int dst_pixel_type, size_t dst_pitch_bytes,
	const cfhip_sdf_params* params, cfhip_sdf_result* results_device, void* stream_)
{
	static_assert(sizeof(cfhip_sdf_params) == 24 && sizeof(cfhip_sdf_result) == 16, "the ABI's sizes");
	return guarded(ctx, "alpha_sdf", [&]() -> int {
		const char* const what = "alpha_sdf";
		CF_TRY(check_given(ctx, what, "params", params));
		CF_TRY(check_given(ctx, what, "src", src));
		CF_TRY(check_given(ctx, what, "dst", dst));
		CF_TRY(check_layers(ctx, what, layers));
		CF_TRY(check_sides(ctx, what, width, height, CFSD_MAX_SIDE));
		size_t spb, dpb;
		CF_TRY(check_pixel_type(ctx, what, "src_pixel_type", src_pixel_type, &spb));
		CF_TRY(check_pixel_type(ctx, what, "dst_pixel_type", dst_pixel_type, &dpb));
		CF_TRY(check_flags(ctx, what, params->flags, CFHIP_SDF_WRAP_X | CFHIP_SDF_WRAP_Y));
		const float t = params->alpha_threshold;
		CF_TRY(check_threshold(ctx, what, t));
		if (params->spread < 1u || params->spread > CFSD_MAX_SPREAD)
			return fail(ctx, CFHIP_E_INVALID, "alpha_sdf: params->spread %u outside 1 to %u", params->spread, CFSD_MAX_SPREAD);
		const uint32_t s = params->scale;
		if (s != 1u && s != 2u && s != 4u && s != 8u && s != 16u)
			return fail(ctx, CFHIP_E_INVALID, "alpha_sdf: params->scale %u is not 1, 2, 4, 8 or 16", s);
		if (!params->channel_mask || params->channel_mask > 15u)
			return fail(ctx, CFHIP_E_INVALID, "alpha_sdf: params->channel_mask 0x%x outside 1 to 15", params->channel_mask);
		if (params->reserved)
			return fail(ctx, CFHIP_E_INVALID, "alpha_sdf: params->reserved is %u, not 0", params->reserved);
		if (width % s || height % s)
			return fail(ctx, CFHIP_E_INVALID, "alpha_sdf: %ux%u is not a multiple of the scale %u", width, height, s);
		CF_TRY(check_row_pitch(ctx, what, "src_pitch_bytes", src_pitch_bytes, (size_t)width*spb));
		CF_TRY(check_pitch_aligned(ctx, what, "src_pitch_bytes", src_pitch_bytes, spb/4u, "a component"));
		CF_TRY(check_row_pitch(ctx, what, "dst_pitch_bytes", dst_pitch_bytes, (size_t)(width/s)*dpb));
		CF_TRY(check_pitch_aligned(ctx, what, "dst_pitch_bytes", dst_pitch_bytes, dpb/4u, "a component"));
		const uint64_t texels = (uint64_t)layers*width*height;
		if (texels > CFSD_MAX_TEXELS)
			return fail(ctx, CFHIP_E_INVALID, "alpha_sdf: more than 2^31 texels in one call");
		for (uint32_t l = 0; l < layers; ++l) {
			CF_TRY(check_item_given(ctx, what, "src", l, src[l]));
			CF_TRY(check_item_given(ctx, what, "dst", l, dst[l]));
			CF_TRY(check_item_aligned(ctx, what, "src", l, src[l], spb/4u, "a component"));
			CF_TRY(check_item_aligned(ctx, what, "dst", l, dst[l], dpb/4u, "a component"));
			// in place: every alpha is read before anything is written, but only a surface of the same geometry is one
			if (dst[l] == src[l] && (s != 1u || dst_pixel_type != src_pixel_type))
				return fail(ctx, CFHIP_E_INVALID, "alpha_sdf: dst[%u] equals src[%u]: in place needs scale 1 and equal pixel types", l, l);
		}
		// d_batch: the layers' source pointers, then their destination pointers.  d_src: the bit plane (whole words per
		// row), e (16 bits per texel, scale > 1 only), the row bytes -- in the order of their alignment
		const size_t plane_bytes = (size_t)layers*height*((width + 63u)/64u)*8u, e_bytes = s > 1u ? (size_t)texels*2u : 0u;
		return device_pass(ctx, stream_, "cfhip_alpha_sdf_column_kernel", (size_t)layers*2u*sizeof(void*),
			plane_bytes + e_bytes + (size_t)texels, [&](hipStream_t stream) -> int {
			void** table[2];
			CF_TRY(upload_tables(ctx, stream, {{src, layers}, {dst, layers}}, table));
			if (results_device)
				HIP_TRY(ctx, hipMemsetAsync(results_device, 0, (size_t)layers*sizeof(cfhip_sdf_result), stream));
			cfsd_call call;
			call.src = table[0];
			call.dst = table[1];
			call.src_pitch = src_pitch_bytes; call.dst_pitch = dst_pitch_bytes;
			call.width = width; call.height = height;
			call.src_type = src_pixel_type; call.dst_type = dst_pixel_type;
			call.flags = params->flags;
			call.spread = params->spread; call.scale = s; call.channel_mask = params->channel_mask;
			uint8_t* scratch = static_cast<uint8_t*>(ctx->d_src);
			uint64_t* plane = reinterpret_cast<uint64_t*>(scratch);
			uint16_t* e = reinterpret_cast<uint16_t*>(scratch + plane_bytes);
			uint8_t* rows = scratch + plane_bytes + e_bytes;
			LaunchChain sdf(ctx, stream, "alpha_sdf");
			sdf([&] { return cfhip_launch_alpha_sdf_classify(&call, layers, t, plane, results_device, stream); });
			sdf([&] { return cfhip_launch_alpha_sdf_row(&call, layers, plane, rows, stream); });
			sdf([&] { return cfhip_launch_alpha_sdf_column(&call, layers, rows, e, results_device, stream); });
			if (s > 1u)
				sdf([&] { return cfhip_launch_alpha_sdf_resolve(&call, layers, e, stream); });
			return sdf.rc;
		});
	});
}

// ---- specular anti-aliasing (csrc/spec_aa.hip): the normals' variance into the levels of a roughness chain -----------
int cfhip_spec_aa_array_device(cfhip_ctx* ctx, const void* const* normals, uint32_t layers, int normal_pixel_type, uint32_t width,
	uint32_t height, size_t normal_pitch_bytes, const void* const* rough0, int rough_pixel_type, size_t rough_pitch_bytes,
	void* const* levels, uint32_t levels_count, const cfhip_spec_aa_params* params, cfhip_spec_aa_result* results_device,
	void* stream_)
{
	static_assert(sizeof(cfhip_spec_aa_params) == 32 && sizeof(cfhip_spec_aa_result) == 16, "the ABI's sizes");
	static_assert(sizeof(cfsa_moments) == 32, "a tile's moments in the scratch");
	static_assert(CFSA_MAX_LAYERS == 65535u, "check_layers' range");
	return guarded(ctx, "spec_aa", [&]() -> int {
		const char* const what = "spec_aa";
		CF_TRY(check_given(ctx, what, "params", params));
		if (params->struct_size != sizeof(cfhip_spec_aa_params))
			return fail(ctx, CFHIP_E_INVALID, "spec_aa: params->struct_size is %u, not %zu", params->struct_size,
				sizeof(cfhip_spec_aa_params));
		CF_TRY(check_given(ctx, what, "normals", normals));
		CF_TRY(check_given(ctx, what, "levels", levels));
		CF_TRY(check_layers(ctx, what, layers));
		CF_TRY(check_sides(ctx, what, width, height, CFSA_MAX_SIDE));
		size_t npb, rpb = 0;
		CF_TRY(check_pixel_type(ctx, what, "normal_pixel_type", normal_pixel_type, &npb));
		if (rough0)
			CF_TRY(check_pixel_type(ctx, what, "rough_pixel_type", rough_pixel_type, &rpb));
		CF_TRY(check_flags(ctx, what, params->flags,
			CFHIP_SPEC_AA_PERCEPTUAL | CFHIP_SPEC_AA_SIGNED_NORMALS | CFHIP_SPEC_AA_RECONSTRUCT_Z));
		if (params->channel > 3u)
			return fail(ctx, CFHIP_E_INVALID, "spec_aa: params->channel %u above 3", params->channel);
		if (!(params->base_roughness >= 0.0f && params->base_roughness <= 1.0f))
			return fail(ctx, CFHIP_E_INVALID, "spec_aa: params->base_roughness %g outside [0, 1]", (double)params->base_roughness);
		if (!(params->variance_scale >= 0.0f) || !std::isfinite(params->variance_scale))
			return fail(ctx, CFHIP_E_INVALID, "spec_aa: params->variance_scale %g is negative or not finite",
				(double)params->variance_scale);
		if (!(params->max_variance >= 0.0f) || !std::isfinite(params->max_variance))
			return fail(ctx, CFHIP_E_INVALID, "spec_aa: params->max_variance %g is negative or not finite",
				(double)params->max_variance);
		if (params->reserved[0] || params->reserved[1])
			return fail(ctx, CFHIP_E_INVALID, "spec_aa: params->reserved is not 0");
		const uint32_t chain = chain_levels(width, height);
		if (levels_count < 2u || levels_count > chain)
			return fail(ctx, CFHIP_E_INVALID, "spec_aa: levels_count %u outside 2 to %u, the chain of %ux%u", levels_count, chain,
				width, height);
		if ((uint64_t)width*height > CFSA_MAX_TEXELS)
			return fail(ctx, CFHIP_E_INVALID, "spec_aa: more than 2^30 texels in level 0");
		CF_TRY(check_row_pitch(ctx, what, "normal_pitch_bytes", normal_pitch_bytes, (size_t)width*npb));
		CF_TRY(check_pitch_aligned(ctx, what, "normal_pitch_bytes", normal_pitch_bytes, npb, "a texel"));
		if (rough0) {
			CF_TRY(check_row_pitch(ctx, what, "rough_pitch_bytes", rough_pitch_bytes, (size_t)width*rpb));
			CF_TRY(check_pitch_aligned(ctx, what, "rough_pitch_bytes", rough_pitch_bytes, rpb/4u, "a component"));
		}
		const uint32_t per = levels_count - 1u;
		for (uint32_t l = 0; l < layers; ++l) {
			CF_TRY(check_item_given(ctx, what, "normals", l, normals[l]));
			CF_TRY(check_item_aligned(ctx, what, "normals", l, normals[l], npb, "a texel"));
			if (rough0) {
				CF_TRY(check_item_given(ctx, what, "rough0", l, rough0[l]));
				CF_TRY(check_item_aligned(ctx, what, "rough0", l, rough0[l], rpb/4u, "a component"));
			}
			for (uint32_t k = 1; k < levels_count; ++k)
				CF_TRY(check_chain_level(ctx, what, levels, per, l, k));
		}
		// d_batch: the layers' normals, their roughness maps (if any), then the levels.  d_src: a launch's last moments
		// are the next one's input -- level 5, then level 10, layer after layer
		const auto dim = [](uint32_t d, uint32_t k) { return (d >> k) ? (d >> k) : 1u; };
		const uint32_t stages = (per + CFSA_STAGE_LEVELS - 1u)/CFSA_STAGE_LEVELS;
		size_t moments[CFSA_MAX_STAGES] = {0, 0, 0};       // moments[s]: what stage s writes
		for (uint32_t s = 0; s + 1u < stages; ++s) {
			const uint32_t k = (s + 1u)*CFSA_STAGE_LEVELS;
			moments[s] = (size_t)layers*dim(width, k)*dim(height, k);
		}
		const size_t nrough = rough0 ? layers : 0u, ntab = (size_t)layers + nrough + (size_t)layers*per;
		return device_pass(ctx, stream_, "cfhip_spec_aa_texel_kernel", ntab*sizeof(void*),
			std::max<size_t>((moments[0] + moments[1])*sizeof(cfsa_moments), 16u), [&](hipStream_t stream) -> int {
			void** table[3];
			CF_TRY(upload_tables(ctx, stream, {{normals, layers}, {rough0, nrough}, {levels, (size_t)layers*per}}, table));
			if (results_device)
				HIP_TRY(ctx, hipMemsetAsync(results_device, 0, (size_t)layers*per*sizeof(cfhip_spec_aa_result), stream));
			cfsa_call call;
			call.normals = table[0];
			call.rough0 = rough0 ? table[1] : nullptr;
			call.levels = table[2];
			call.normal_pitch = normal_pitch_bytes;
			call.rough_pitch = rough0 ? rough_pitch_bytes : 0u;
			call.width = width; call.height = height;
			call.levels_count = levels_count;
			call.normal_type = normal_pixel_type;
			call.rough_type = rough0 ? rough_pixel_type : 0;
			call.flags = params->flags;
			call.channel = params->channel;
			call.base_roughness = params->base_roughness;
			call.variance_scale = params->variance_scale;
			call.max_variance = params->max_variance;
			cfsa_moments* const m0 = static_cast<cfsa_moments*>(ctx->d_src);
			cfsa_moments* const buf[CFSA_MAX_STAGES] = {m0, m0 + moments[0], nullptr};
			LaunchChain spec(ctx, stream, "spec_aa");
			for (uint32_t s = 0; s < stages; ++s)
				spec([&] {
					return cfhip_launch_spec_aa(&call, layers, s, s ? buf[s - 1u] : nullptr, s + 1u < stages ? buf[s] : nullptr,
						results_device, stream);
				});
			return spec.rc;
		});
	});
}

// ---- ambient occlusion from height maps (csrc/height_ao.hip): the horizon in D directions within R texels -------------
// The first quadrant of each direction set and its weights: half the angle between a direction's neighbours over 2 pi,
// as the nearest double -- but (1,0) and (3,1) of D = 32, one unit in the last place above it, so that every set sums to
// exactly 1.0 in direction order and a flat surface comes out as exactly 1.
// The other quadrants are these turned by (x, y) -> (-y, x), with the same weights.
namespace {
struct HaoBase {
	int32_t vx, vy;
	double weight;
};
const HaoBase kHaoBase8[2] = {{1, 0, 0.125}, {1, 1, 0.125}};
const HaoBase kHaoBase16[4] = {{1, 0, 0.07379180882521663}, {2, 1, 0.0625}, {1, 1, 0.05120819117478336}, {1, 2, 0.0625}};
const HaoBase kHaoBase32[8] = {{1, 0, 0.05120819117478337}, {3, 1, 0.03689590441260832}, {2, 1, 0.021187664865358023},
	{3, 2, 0.02560409558739168}, {1, 1, 0.03141647909450059}, {2, 3, 0.02560409558739168}, {1, 2, 0.021187664865358023},
	{1, 3, 0.036895904412608316}};

const HaoBase* hao_base(uint32_t directions)
{
	return directions == 8u ? kHaoBase8 : directions == 16u ? kHaoBase16 : directions == 32u ? kHaoBase32 : nullptr;
}

// direction d of a set
HaoBase hao_direction(const HaoBase* base, uint32_t directions, uint32_t d)
{
	HaoBase v = base[d % (directions/4u)];
	for (uint32_t q = d/(directions/4u); q; --q) {
		const int32_t x = v.vx;
		v.vx = -v.vy;
		v.vy = x;
	}
	return v;
}

// The call's table, in double on the host: every direction's reach R_d and its gains g(d, 1 ... R_d)
void hao_fill_table(cfhao_table* t, uint32_t directions, uint32_t radius, bool falloff)
{
	const HaoBase* base = hao_base(directions);
	uint32_t first = 0;
	for (uint32_t d = 0; d < directions; ++d) {
		const HaoBase v = hao_direction(base, directions, d);
		const uint32_t n = (uint32_t)(v.vx*v.vx + v.vy*v.vy);
		uint32_t reach = 0;
		while ((reach + 1u)*(reach + 1u)*n <= radius*radius)
			++reach;
		const double len = std::sqrt((double)n);
		for (uint32_t k = 1; k <= reach; ++k) {
			double g = 1.0/((double)k*len);
			if (falloff)
				g = g*(1.0 - (double)(k*k*n)/(double)((radius + 1u)*(radius + 1u)));
			t->gain[first + k - 1u] = g;
		}
		t->dir[d] = cfhao_dir{v.vx, v.vy, reach, first, v.weight};
		first += reach;
	}
}
} // namespace

int cfhip_height_ao_directions(uint32_t directions, int32_t* vx, int32_t* vy, double* weight)
{
	const HaoBase* base = hao_base(directions);
	if (!base)
		return CFHIP_E_INVALID;
	for (uint32_t d = 0; d < directions; ++d) {
		const HaoBase v = hao_direction(base, directions, d);
		if (vx) vx[d] = v.vx;
		if (vy) vy[d] = v.vy;
		if (weight) weight[d] = v.weight;
	}
	return CFHIP_OK;
}

int cfhip_height_ao_array_device(cfhip_ctx* ctx, const void* const* src, uint32_t layers, int src_pixel_type, uint32_t width,
	uint32_t height, size_t src_pitch_bytes, void* const* dst, int dst_pixel_type, size_t dst_pitch_bytes,
	const cfhip_height_ao_params* params, cfhip_height_ao_result* results_device, void* stream_)
{
	static_assert(sizeof(cfhip_height_ao_params) == 40 && sizeof(cfhip_height_ao_result) == 16, "the ABI's sizes");
	static_assert(CFHAO_MAX_LAYERS == 65535u, "check_layers' range");
	static_assert(sizeof(cfhao_dir) == 24 && sizeof(cfhao_table) % 8u == 0, "the table the scan reads");
	return guarded(ctx, "height_ao", [&]() -> int {
		const char* const what = "height_ao";
		CF_TRY(check_given(ctx, what, "params", params));
		if (params->struct_size != sizeof(cfhip_height_ao_params))
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->struct_size is %u, not %zu", params->struct_size,
				sizeof(cfhip_height_ao_params));
		CF_TRY(check_given(ctx, what, "src", src));
		CF_TRY(check_given(ctx, what, "dst", dst));
		CF_TRY(check_layers(ctx, what, layers));
		CF_TRY(check_sides(ctx, what, width, height, CFHAO_MAX_SIDE));
		size_t spb, dpb;
		CF_TRY(check_pixel_type(ctx, what, "src_pixel_type", src_pixel_type, &spb));
		CF_TRY(check_pixel_type(ctx, what, "dst_pixel_type", dst_pixel_type, &dpb));
		CF_TRY(check_flags(ctx, what, params->flags,
			CFHIP_HAO_WRAP_X | CFHIP_HAO_WRAP_Y | CFHIP_HAO_UNIFORM | CFHIP_HAO_FALLOFF));
		if (params->channel > 3u)
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->channel %u above 3", params->channel);
		if (!hao_base(params->directions))
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->directions %u is not 8, 16 or 32", params->directions);
		if (params->radius < 1u || params->radius > CFHAO_MAX_RADIUS)
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->radius %u outside 1 to %u", params->radius, CFHAO_MAX_RADIUS);
		if (!params->channel_mask || params->channel_mask > 15u)
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->channel_mask 0x%x outside 1 to 15", params->channel_mask);
		if (!std::isfinite(params->height))
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->height %g is not finite", (double)params->height);
		if (!(params->strength >= 0.0f) || !std::isfinite(params->strength))
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->strength %g is negative or not finite", (double)params->strength);
		if (!(params->bias >= 0.0f) || !std::isfinite(params->bias))
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->bias %g is negative or not finite", (double)params->bias);
		if (params->reserved)
			return fail(ctx, CFHIP_E_INVALID, "height_ao: params->reserved is %u, not 0", params->reserved);
		if ((uint64_t)width*height > CFHAO_MAX_TEXELS)
			return fail(ctx, CFHIP_E_INVALID, "height_ao: more than 2^30 texels in a surface");
		CF_TRY(check_row_pitch(ctx, what, "src_pitch_bytes", src_pitch_bytes, (size_t)width*spb));
		CF_TRY(check_pitch_aligned(ctx, what, "src_pitch_bytes", src_pitch_bytes, spb/4u, "a component"));
		CF_TRY(check_row_pitch(ctx, what, "dst_pitch_bytes", dst_pitch_bytes, (size_t)width*dpb));
		CF_TRY(check_pitch_aligned(ctx, what, "dst_pitch_bytes", dst_pitch_bytes, dpb/4u, "a component"));
		for (uint32_t l = 0; l < layers; ++l) {
			CF_TRY(check_item_given(ctx, what, "src", l, src[l]));
			CF_TRY(check_item_given(ctx, what, "dst", l, dst[l]));
			CF_TRY(check_item_aligned(ctx, what, "src", l, src[l], spb/4u, "a component"));
			CF_TRY(check_item_aligned(ctx, what, "dst", l, dst[l], dpb/4u, "a component"));
			// in place: every height is read before anything is written, but only a surface of the same geometry is one
			if (dst[l] == src[l] && dst_pixel_type != src_pixel_type)
				return fail(ctx, CFHIP_E_INVALID, "height_ao: dst[%u] equals src[%u]: in place needs equal pixel types", l, l);
		}
		// d_batch: the layers' source pointers, their destination pointers, then the call's table.  d_src: the plane,
		// one float per texel, layer after layer
		const size_t tab_bytes = (size_t)layers*2u*sizeof(void*);
		return device_pass(ctx, stream_, "cfhip_height_ao_scan_kernel", tab_bytes + sizeof(cfhao_table),
			(size_t)layers*width*height*sizeof(float), [&](hipStream_t stream) -> int {
			void** table[2];
			CF_TRY(upload_tables(ctx, stream, {{src, layers}, {dst, layers}}, table));
			// (a pageable source, as the pointer tables are: the runtime stages the copy before it returns)
			cfhao_table host;
			std::memset(&host, 0, sizeof(host));
			hao_fill_table(&host, params->directions, params->radius, params->flags & CFHIP_HAO_FALLOFF);
			cfhao_table* const dtab = reinterpret_cast<cfhao_table*>(static_cast<uint8_t*>(ctx->d_batch) + tab_bytes);
			HIP_TRY(ctx, hipMemcpyAsync(dtab, &host, sizeof(host), hipMemcpyHostToDevice, stream));
			cfhao_call call;
			call.src = table[0];
			call.dst = table[1];
			call.table = dtab;
			call.src_pitch = src_pitch_bytes; call.dst_pitch = dst_pitch_bytes;
			call.width = width; call.height = height;
			call.src_type = src_pixel_type; call.dst_type = dst_pixel_type;
			call.flags = params->flags; call.channel = params->channel;
			call.directions = params->directions; call.radius = params->radius; call.channel_mask = params->channel_mask;
			call.height_scale = params->height; call.strength = params->strength; call.bias = params->bias;
			float* const plane = static_cast<float*>(ctx->d_src);
			LaunchChain ao(ctx, stream, "height_ao");
			ao([&] { return cfhip_launch_height_ao_plane(&call, layers, plane, results_device, stream); });
			ao([&] { return cfhip_launch_height_ao_scan(&call, layers, plane, results_device, stream); });
			return ao.rc;
		});
	});
}

// ---- environment maps (csrc/envmap.hip): panorama to cube, the GGX chain, nine SH coefficients ------------------------
int cfhip_equirect_to_cube_device(cfhip_ctx* ctx, const void* src, int src_pixel_type, uint32_t width, uint32_t height,
	size_t src_pitch_bytes, void* const* faces, uint32_t face_size, uint32_t supersample, void* stream_)
{
	return guarded(ctx, "equirect_to_cube", [&]() -> int {
		const char* const what = "equirect_to_cube";
		CF_TRY(check_given(ctx, what, "src", src));
		if (width < 2u || !height || width > CFENV_MAX_PANORAMA || height > CFENV_MAX_PANORAMA)
			return fail(ctx, CFHIP_E_INVALID, "equirect_to_cube: width is 2 to %u and height 1 to %u, not %ux%u", CFENV_MAX_PANORAMA,
				CFENV_MAX_PANORAMA, width, height);
		size_t spb;
		CF_TRY(check_pixel_type(ctx, what, "src_pixel_type", src_pixel_type, &spb));
		CF_TRY(check_row_pitch(ctx, what, "src_pitch_bytes", src_pitch_bytes, (size_t)width*spb));
		CF_TRY(check_pitch_aligned(ctx, what, "src_pitch_bytes", src_pitch_bytes, spb/4u, "a component"));
		if ((uintptr_t)src % (spb/4u))
			return fail(ctx, CFHIP_E_INVALID, "equirect_to_cube: src not aligned to a component (%zu bytes)", spb/4u);
		if (supersample != 1u && supersample != 2u && supersample != 4u)
			return fail(ctx, CFHIP_E_INVALID, "equirect_to_cube: supersample %u is not 1, 2 or 4", supersample);
		CF_TRY(check_faces(ctx, what, faces, face_size));
		for (uint32_t f = 0; f < 6u; ++f)
			if (faces[f] == src)
				return fail(ctx, CFHIP_E_INVALID, "equirect_to_cube: faces[%u] equals src", f);
		return device_pass(ctx, stream_, "cfhip_equirect_to_cube_kernel", 6u*sizeof(void*), 0, [&](hipStream_t stream) -> int {
			void** table[1];
			CF_TRY(upload_tables(ctx, stream, {{faces, 6u}}, table));
			return timed(ctx, stream, "equirect_to_cube", [&] {
				return cfhip_launch_equirect_to_cube(src, src_pixel_type, width, height, src_pitch_bytes, table[0], face_size,
					supersample, stream);
			});
		});
	});
}

// the second Hammersley coordinate of point i: the 32 bits of i reversed, times 2^-32
static double radical_inverse(uint32_t i)
{
	uint32_t bits = i;
	bits = (bits << 16) | (bits >> 16);
	bits = ((bits & 0x00FF00FFu) << 8) | ((bits & 0xFF00FF00u) >> 8);
	bits = ((bits & 0x0F0F0F0Fu) << 4) | ((bits & 0xF0F0F0F0u) >> 4);
	bits = ((bits & 0x33333333u) << 2) | ((bits & 0xCCCCCCCCu) >> 2);
	bits = ((bits & 0x55555555u) << 1) | ((bits & 0xAAAAAAAAu) >> 1);
	return (double)bits*0x1p-32;
}

// what every sample table takes: a multiple of 64 records, a face and the levels of its source chain
static bool table_shape_ok(uint32_t samples, uint32_t face_size, uint32_t source_levels)
{
	if (samples % 64u || samples < CFENV_MIN_SAMPLES || samples > CFENV_MAX_SAMPLES)
		return false;
	return face_size && face_size <= CFENV_MAX_FACE && source_levels && source_levels <= cube_levels(face_size);
}

int cfhip_ggx_sample_table(float roughness, uint32_t samples, uint32_t face_size, uint32_t source_levels, cfhip_ggx_sample* out)
{
	if (!out || !(roughness > 0.0f && roughness <= 1.0f))
		return CFHIP_E_INVALID;
	if (!table_shape_ok(samples, face_size, source_levels))
		return CFHIP_E_INVALID;
	const double S = (double)samples, N = (double)face_size, r = (double)roughness;
	const double a = r*r, a2 = a*a;
	for (uint32_t i = 0; i < samples; ++i) {
		const double xi1 = ((double)i + 0.5)/S, xi2 = radical_inverse(i);
		const double cos2 = (1.0 - xi1)/(1.0 + (a2 - 1.0)*xi1);
		const double hz = std::sqrt(cos2), sine = std::sqrt(1.0 - cos2), phi = (2.0*CFENV_PI)*xi2;
		const double hx = sine*std::cos(phi), hy = sine*std::sin(phi);
		const double lx = (2.0*hz)*hx, ly = (2.0*hz)*hy;
		double lz = (2.0*hz)*hz - 1.0;
		const double e = (hz*hz)*(a2 - 1.0) + 1.0;
		const double pdf = (a2/(CFENV_PI*(e*e)))/4.0;
		double lod = 0.5*std::log2((1.0/(S*pdf))/((4.0*CFENV_PI)/(6.0*(N*N)))) + 1.0;
		lod = std::fmin(std::fmax(lod, 0.0), (double)(source_levels - 1u));
		if (lz <= 0.0) {
			lz = 0.0;
			lod = 0.0;
		}
		out[i].lx = (float)lx; out[i].ly = (float)ly; out[i].lz = (float)lz; out[i].lod = (float)lod;
	}
	return CFHIP_OK;
}

int cfhip_cube_prefilter_device(cfhip_ctx* ctx, const void* const* src_levels, uint32_t face_size, uint32_t source_levels,
	void* const* dst_levels, uint32_t dst_count, const cfhip_ggx_sample* const* tables, const uint32_t* table_samples,
	void* stream_)
{
	static_assert(sizeof(cfhip_ggx_sample) == 16 && sizeof(cfhip_sh9_result) == 296, "the ABI's sizes");
	return guarded(ctx, "cube_prefilter", [&]() -> int {
		const char* const what = "cube_prefilter";
		CF_TRY(check_given(ctx, what, "src_levels", src_levels));
		CF_TRY(check_given(ctx, what, "dst_levels", dst_levels));
		CF_TRY(check_given(ctx, what, "tables", tables));
		CF_TRY(check_given(ctx, what, "table_samples", table_samples));
		if (!face_size || face_size > CFENV_MAX_FACE)
			return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: face_size is 1 to %u, not %u", CFENV_MAX_FACE, face_size);
		const uint32_t full = cube_levels(face_size);
		if (!source_levels || source_levels > full)
			return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: source_levels is 1 to %u for a face of %u, not %u", full, face_size,
				source_levels);
		if (!dst_count || dst_count > full)
			return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: dst_count is 1 to %u for a face of %u, not %u", full, face_size, dst_count);
		// (the two-index texts of these lists are this pass's own)
		for (uint32_t i = 0; i < 6u*source_levels; ++i) {
			if (!src_levels[i])
				return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: src_levels[%u][%u] is NULL", i/source_levels, i%source_levels);
			if ((uintptr_t)src_levels[i] % 16u)
				return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: src_levels[%u][%u] not aligned to a texel (16 bytes)", i/source_levels,
					i%source_levels);
		}
		for (uint32_t i = 0; i < 6u*dst_count; ++i) {
			if (!dst_levels[i])
				return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: dst_levels[%u][%u] is NULL", i/dst_count, i%dst_count);
			if ((uintptr_t)dst_levels[i] % 16u)
				return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: dst_levels[%u][%u] not aligned to a texel (16 bytes)", i/dst_count,
					i%dst_count);
			for (uint32_t j = 0; j < 6u*source_levels; ++j)
				if (dst_levels[i] == src_levels[j])
					return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: dst_levels[%u][%u] equals src_levels[%u][%u]", i/dst_count,
						i%dst_count, j/source_levels, j%source_levels);
		}
		size_t records = 0;
		for (uint32_t k = 0; k < dst_count; ++k) {
			const uint32_t S = table_samples[k];
			if (!S) {
				if (k >= source_levels)
					return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: table_samples[%u] is 0, a copy, but there are %u source levels", k,
						source_levels);
				continue;
			}
			if (S % 64u || S < CFENV_MIN_SAMPLES || S > CFENV_MAX_SAMPLES)
				return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: table_samples[%u] is %u, not 0 or a multiple of 64 from %u to %u", k, S,
					CFENV_MIN_SAMPLES, CFENV_MAX_SAMPLES);
			CF_TRY(check_item_given(ctx, what, "tables", k, tables[k]));
			for (uint32_t i = 0; i < S; ++i) {
				const cfhip_ggx_sample& r = tables[k][i];
				if (!(std::isfinite(r.lx) && std::isfinite(r.ly) && r.lz >= 0.0f && std::isfinite(r.lz) && r.lod >= 0.0f &&
					  r.lod <= (float)CFENV_MAX_LEVELS))
					return fail(ctx, CFHIP_E_INVALID, "cube_prefilter: tables[%u][%u] is not finite with lz >= 0 and 0 <= lod <= %u", k, i,
						CFENV_MAX_LEVELS);
			}
			records += S;
		}
		// d_batch: the source chain's pointers, then the destination's.  d_src: the levels' tables, one after the other
		const size_t ns = 6u*(size_t)source_levels, nd = 6u*(size_t)dst_count;
		return device_pass(ctx, stream_, "cfhip_cube_prefilter_kernel", (ns + nd)*sizeof(void*), records*sizeof(cfhip_ggx_sample),
			[&](hipStream_t stream) -> int {
			void** table[2];
			CF_TRY(upload_tables(ctx, stream, {{src_levels, ns}, {dst_levels, nd}}, table));
			cfhip_ggx_sample* d_tables = static_cast<cfhip_ggx_sample*>(ctx->d_src);
			size_t at = 0;
			for (uint32_t k = 0; k < dst_count; ++k)
				if (table_samples[k]) {
					HIP_TRY(ctx, hipMemcpyAsync(d_tables + at, tables[k], (size_t)table_samples[k]*sizeof(cfhip_ggx_sample),
						hipMemcpyHostToDevice, stream));
					at += table_samples[k];
				}
			cfenv_prefilter_call call;
			call.src = table[0];
			call.dst = table[1];
			call.face_size = face_size; call.src_levels = source_levels; call.dst_levels = dst_count;
			at = 0;
			// every level is a timed span of its own
			LaunchChain level(ctx, stream, "cube_prefilter");
			for (uint32_t k = 0; k < dst_count; ++k) {
				call.level = k;
				call.samples = table_samples[k];
				call.table = d_tables + at;
				at += table_samples[k];
				level([&] { return cfhip_launch_cube_prefilter(&call, stream); });
			}
			return level.rc;
		});
	});
}

int cfhip_cube_sh9_device(cfhip_ctx* ctx, const void* const* faces, uint32_t face_size, cfhip_sh9_result* result_device,
	void* stream_)
{
	return guarded(ctx, "cube_sh9", [&]() -> int {
		CF_TRY(check_faces(ctx, "cube_sh9", faces, face_size));
		CF_TRY(check_given(ctx, "cube_sh9", "result_device", result_device));
		if ((uintptr_t)result_device % 8u)
			return fail(ctx, CFHIP_E_INVALID, "cube_sh9: result_device not aligned to 8 bytes");
		// d_batch: the six pointers.  d_src: a record of 37 doubles per face row
		return device_pass(ctx, stream_, "cfhip_cube_sh9_rows_kernel", 6u*sizeof(void*),
			6u*(size_t)face_size*CFENV_SH_VALUES*sizeof(double), [&](hipStream_t stream) -> int {
			void** table[1];
			CF_TRY(upload_tables(ctx, stream, {{faces, 6u}}, table));
			double* rows = static_cast<double*>(ctx->d_src);
			LaunchChain sh9(ctx, stream, "cube_sh9");
			sh9([&] { return cfhip_launch_cube_sh9_rows(table[0], face_size, rows, stream); });
			sh9([&] { return cfhip_launch_cube_sh9_final(rows, face_size, result_device, stream); });
			return sh9.rc;
		});
	});
}

// ---- the other lobes' tables, the BRDF lookup table, the irradiance cube (csrc/envmap.hip) ------
int cfhip_lobe_sample_table(int kind, float roughness, uint32_t samples, uint32_t face_size, uint32_t source_levels,
	cfhip_ggx_sample* out)
{
	if (kind == CFENV_LOBE_GGX)
		return cfhip_ggx_sample_table(roughness, samples, face_size, source_levels, out);
	if (kind != CFENV_LOBE_CHARLIE && kind != CFENV_LOBE_LAMBERT)
		return CFHIP_E_INVALID;
	if (!out || !table_shape_ok(samples, face_size, source_levels))
		return CFHIP_E_INVALID;
	if (kind == CFENV_LOBE_CHARLIE && !(roughness > 0.0f && roughness <= 1.0f))
		return CFHIP_E_INVALID;
	const double S = (double)samples, N = (double)face_size, r = (double)roughness;
	const double a = r*r;
	for (uint32_t i = 0; i < samples; ++i) {
		const double xi1 = ((double)i + 0.5)/S, xi2 = radical_inverse(i);
		const double phi = (2.0*CFENV_PI)*xi2;
		double lx, ly, lz, pdf;
		if (kind == CFENV_LOBE_CHARLIE) {
			const double sine = std::pow(xi1, a/(2.0*a + 1.0)), hz = std::sqrt(1.0 - sine*sine);
			const double hx = sine*std::cos(phi), hy = sine*std::sin(phi);
			lx = (2.0*hz)*hx;
			ly = (2.0*hz)*hy;
			lz = (2.0*hz)*hz - 1.0;
			pdf = (((2.0 + 1.0/a)*std::pow(sine, 1.0/a))/(2.0*CFENV_PI))/4.0;
		} else {
			lz = 1.0 - xi1;
			const double sine = std::sqrt(1.0 - lz*lz);
			lx = sine*std::cos(phi);
			ly = sine*std::sin(phi);
			pdf = 1.0/(2.0*CFENV_PI);
		}
		double lod = 0.5*std::log2((1.0/(S*pdf))/((4.0*CFENV_PI)/(6.0*(N*N)))) + 1.0;
		lod = std::fmin(std::fmax(lod, 0.0), (double)(source_levels - 1u));
		if (lz <= 0.0) {
			lz = 0.0;
			lod = 0.0;
		}
		out[i].lx = (float)lx; out[i].ly = (float)ly; out[i].lz = (float)lz; out[i].lod = (float)lod;
	}
	return CFHIP_OK;
}

int cfhip_hammersley_table(uint32_t samples, cfhip_hammersley_sample* out)
{
	if (!out || !table_shape_ok(samples, 1u, 1u))
		return CFHIP_E_INVALID;
	const double S = (double)samples;
	for (uint32_t i = 0; i < samples; ++i) {
		const double phi = (2.0*CFENV_PI)*radical_inverse(i);
		out[i].cos_phi = (float)std::cos(phi); out[i].sin_phi = (float)std::sin(phi);
		out[i].xi1 = (float)(((double)i + 0.5)/S); out[i].reserved = 0.0f;
	}
	return CFHIP_OK;
}

int cfhip_brdf_lut_device(cfhip_ctx* ctx, void* dst, uint32_t width, uint32_t height, const cfhip_hammersley_sample* table,
	uint32_t samples, uint32_t sheen, void* stream_)
{
	static_assert(sizeof(cfhip_hammersley_sample) == 16, "the ABI's sizes");
	return guarded(ctx, "brdf_lut", [&]() -> int {
		const char* const what = "brdf_lut";
		CF_TRY(check_given(ctx, what, "dst", dst));
		if ((uintptr_t)dst % 16u)
			return fail(ctx, CFHIP_E_INVALID, "brdf_lut: dst not aligned to a texel (16 bytes)");
		CF_TRY(check_sides(ctx, what, width, height, CFENV_MAX_LUT));
		CF_TRY(check_given(ctx, what, "table", table));
		if (samples % 64u || samples < CFENV_MIN_SAMPLES || samples > CFENV_MAX_SAMPLES)
			return fail(ctx, CFHIP_E_INVALID, "brdf_lut: samples is %u, not a multiple of 64 from %u to %u", samples,
				CFENV_MIN_SAMPLES, CFENV_MAX_SAMPLES);
		if (sheen > 1u)
			return fail(ctx, CFHIP_E_INVALID, "brdf_lut: sheen is 0 or 1, not %u", sheen);
		for (uint32_t i = 0; i < samples; ++i) {
			const cfhip_hammersley_sample& r = table[i];
			if (!(std::isfinite(r.cos_phi) && std::isfinite(r.sin_phi) && r.xi1 > 0.0f && r.xi1 < 1.0f))
				return fail(ctx, CFHIP_E_INVALID, "brdf_lut: table[%u] is not finite with 0 < xi1 < 1", i);
		}
		// d_src: the table
		return device_pass(ctx, stream_, "cfhip_brdf_lut_kernel", 0, (size_t)samples*sizeof(cfhip_hammersley_sample),
			[&](hipStream_t stream) -> int {
			cfhip_hammersley_sample* d_table = static_cast<cfhip_hammersley_sample*>(ctx->d_src);
			HIP_TRY(ctx, hipMemcpyAsync(d_table, table, (size_t)samples*sizeof(cfhip_hammersley_sample), hipMemcpyHostToDevice,
				stream));
			return timed(ctx, stream, "brdf_lut", [&] { return cfhip_launch_brdf_lut(dst, width, height, d_table, samples, sheen, stream); });
		});
	});
}

int cfhip_cube_irradiance_device(cfhip_ctx* ctx, const cfhip_sh9_result* sh9_result_device, void* const* faces,
	uint32_t face_size, uint32_t over_pi, void* stream_)
{
	return guarded(ctx, "cube_irradiance", [&]() -> int {
		const char* const what = "cube_irradiance";
		CF_TRY(check_given(ctx, what, "sh9_result_device", sh9_result_device));
		if ((uintptr_t)sh9_result_device % 8u)
			return fail(ctx, CFHIP_E_INVALID, "cube_irradiance: sh9_result_device not aligned to 8 bytes");
		CF_TRY(check_faces(ctx, what, faces, face_size));
		for (uint32_t f = 0; f < 6u; ++f)
			if (faces[f] == sh9_result_device)
				return fail(ctx, CFHIP_E_INVALID, "cube_irradiance: faces[%u] equals sh9_result_device", f);
		if (over_pi > 1u)
			return fail(ctx, CFHIP_E_INVALID, "cube_irradiance: over_pi is 0 or 1, not %u", over_pi);
		return device_pass(ctx, stream_, "cfhip_cube_irradiance_kernel", 6u*sizeof(void*), 0, [&](hipStream_t stream) -> int {
			void** table[1];
			CF_TRY(upload_tables(ctx, stream, {{faces, 6u}}, table));
			return timed(ctx, stream, "cube_irradiance", [&] {
				return cfhip_launch_cube_irradiance(sh9_result_device, table[0], face_size, over_pi, stream);
			});
		});
	});
}

int cfhip_resize_device(cfhip_ctx* ctx, const void* src, int src_pixel_type, uint32_t src_width,
	uint32_t src_height, size_t src_pitch_bytes, int color_space, int filter, void* dst,
	uint32_t dst_width, uint32_t dst_height, void* stream_)
{
	return guarded(ctx, "resize", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		if (!src || !dst || !src_width || !src_height || !dst_width || !dst_height)
			return fail(ctx, CFHIP_E_INVALID, "resize: NULL or empty argument");
		int rc = check_mip_args(ctx, "resize", src_pixel_type, color_space, filter, src_width, src_height, 0, 1,
			src_pitch_bytes);
		if (rc != CFHIP_OK)
			return rc;
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		if (src_width == dst_width && src_height == dst_height) {
			// Image::resize returns the image itself (Image.cpp:1330-1334): the texels as RGBAF, no
			// colour-space round trip (a 1:1 box footprint is the texel)
			HIP_TRY(ctx, cfhip_launch_mip_resize(src, src_pixel_type, src_pitch_bytes, src_width, src_height, dst,
				dst_width, dst_height, CFHIP_FILTER_BOX, 0, lease.stream));
		} else {
			rc = mip_level_2d(ctx, lease, src, src_pixel_type, src_pitch_bytes, src_width, src_height, dst,
				dst_width, dst_height, filter, color_space == CFHIP_COLOR_SRGB ? 1 : 0);
			if (rc != CFHIP_OK)
				return rc;
		}
		return lease.done(!stream_);
	});
}

// Image's pixel operations (csrc/image_ops.hip).  No staging buffer is touched, so no StagingLease: the call
// only follows the stream rule itself.
int cfhip_image_ops_device(cfhip_ctx* ctx, const void* src, int src_pixel_type, uint32_t w, uint32_t h,
	size_t src_pitch_bytes, const cfhip_image_ops* ops, void* dst, size_t dst_pitch_bytes, void* stream_)
{
	return guarded(ctx, "image ops", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		if (!src || !dst || !ops)
			return fail(ctx, CFHIP_E_INVALID, "image ops: src, dst or ops is NULL");
		if (!w || !h)
			return fail(ctx, CFHIP_E_INVALID, "image ops: empty image %ux%u", w, h);
		if (w > (1u << 20) || h > (1u << 20))
			return fail(ctx, CFHIP_E_INVALID, "image ops: image %ux%u too large for one launch", w, h);
		if (src_pixel_type < CFHIP_PIXEL_RGBA8 || src_pixel_type > CFHIP_PIXEL_RGBA16F)
			return fail(ctx, CFHIP_E_INVALID, "image ops: pixel type %d", src_pixel_type);
		const uint32_t all_ops = CFHIP_IMAGE_OP_COLOR_SPACE | CFHIP_IMAGE_OP_ROTATE | CFHIP_IMAGE_OP_GRAYSCALE |
			CFHIP_IMAGE_OP_NORMAL_MAP | CFHIP_IMAGE_OP_FLIP_X | CFHIP_IMAGE_OP_FLIP_Y | CFHIP_IMAGE_OP_SWIZZLE |
			CFHIP_IMAGE_OP_PREMULTIPLY;
		if (ops->ops & ~all_ops)
			return fail(ctx, CFHIP_E_INVALID, "image ops: unknown op bits 0x%x", ops->ops & ~all_ops);
		for (int cs : {ops->src_color_space, ops->dst_color_space})
			if (cs != CFHIP_COLOR_LINEAR && cs != CFHIP_COLOR_SRGB)
				return fail(ctx, CFHIP_E_INVALID, "image ops: colour space %d", cs);
		if (ops->rotate < CFHIP_ROTATE_CW90 || ops->rotate > CFHIP_ROTATE_CCW270)
			return fail(ctx, CFHIP_E_INVALID, "image ops: rotate angle %d", ops->rotate);
		if (ops->normal_options & ~(uint32_t)(CFHIP_NORMAL_KEEP_SIGN | CFHIP_NORMAL_WRAP_X | CFHIP_NORMAL_WRAP_Y))
			return fail(ctx, CFHIP_E_INVALID, "image ops: normal options 0x%x", ops->normal_options);
		for (int c = 0; c < 4; ++c)
			if (ops->swizzle[c] < CFHIP_CHANNEL_RED || ops->swizzle[c] > CFHIP_CHANNEL_NONE)
				return fail(ctx, CFHIP_E_INVALID, "image ops: swizzle[%d] channel %d", c, ops->swizzle[c]);
		if (ops->rgbf > 1u)
			return fail(ctx, CFHIP_E_INVALID, "image ops: rgbf flag %u", ops->rgbf);
		const size_t pb = pixel_bytes(src_pixel_type);
		const bool quarter = (ops->ops & CFHIP_IMAGE_OP_ROTATE) && ops->rotate != CFHIP_ROTATE_CW180 &&
			ops->rotate != CFHIP_ROTATE_CCW180;
		const uint32_t rw = quarter ? h : w, rh = quarter ? w : h;
		if (src_pitch_bytes < (size_t)w*pb)
			return fail(ctx, CFHIP_E_INVALID, "image ops: source pitch %zu < %zu", src_pitch_bytes, (size_t)w*pb);
		if (dst_pitch_bytes < (size_t)rw*16u)
			return fail(ctx, CFHIP_E_INVALID, "image ops: destination pitch %zu < %zu", dst_pitch_bytes, (size_t)rw*16u);
		// the kernel loads whole texels and stores float4
		if ((uintptr_t)src % pb || src_pitch_bytes % pb || (uintptr_t)dst % 16u || dst_pitch_bytes % 16u)
			return fail(ctx, CFHIP_E_INVALID, "image ops: src / dst or a pitch not aligned to its texel size");
		const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (size_t)(h - 1u)*src_pitch_bytes + (size_t)w*pb;
		const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (size_t)(rh - 1u)*dst_pitch_bytes + (size_t)rw*16u;
		if (s0 < d1 && d0 < s1)
			return fail(ctx, CFHIP_E_INVALID, "image ops: src and dst overlap");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		const hipStream_t stream = call_stream(ctx, stream_);
		begin_call(ctx, stream, "cfhip_image_ops_kernel");
		const int rc = timed(ctx, stream, "image ops", [&] {
			return cfhip_launch_image_ops(src, src_pixel_type, src_pitch_bytes, w, h, ops, dst, dst_pitch_bytes, stream);
		});
		if (rc != CFHIP_OK)
			return rc;
		if (!stream_)
			HIP_TRY(ctx, hipStreamSynchronize(stream));
		return CFHIP_OK;
	});
}

int cfhip_generate_mips3d_device(cfhip_ctx* ctx, const void* src, int src_pixel_type,
	uint32_t width, uint32_t height, uint32_t depth, size_t src_pitch_bytes, size_t src_slice_pitch_bytes,
	int color_space, int filter, void* const* dst_levels, uint32_t levels, void* stream_)
{
	return guarded(ctx, "3-D mip generation", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		if (!src || !width || !height || !depth || !levels || (levels > 1 && !dst_levels))
			return fail(ctx, CFHIP_E_INVALID, "3-D mip generation: NULL or empty argument");
		int rc = check_mip_args(ctx, "3-D mip generation", src_pixel_type, color_space, filter, width, height, depth,
			levels, src_pitch_bytes);
		if (rc != CFHIP_OK)
			return rc;
		if (src_slice_pitch_bytes < src_pitch_bytes*height)
			return fail(ctx, CFHIP_E_INVALID, "3-D mip generation: slice pitch smaller than a slice");
		for (uint32_t k = 1; k < levels; ++k)
			if (!dst_levels[k - 1])
				return fail(ctx, CFHIP_E_INVALID, "3-D mip generation: dst_levels[%u] is NULL", k - 1);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		const hipStream_t stream = lease.stream;
		const int srgb = color_space == CFHIP_COLOR_SRGB ? 1 : 0;
		// level k (Texture.cpp:1345-1402): every slice of level k-1 is resized to the level's width and
		// height with Image::resize, then generateMips3d interpolates the slices along the depth
		const uint8_t* prev = static_cast<const uint8_t*>(src);
		int prev_type = src_pixel_type;
		size_t prev_pitch = src_pitch_bytes, prev_slice = src_slice_pitch_bytes;
		uint32_t pw = width, ph = height, pd = depth;
		for (uint32_t k = 1; k < levels; ++k) {
			const uint32_t w = (width >> k) ? (width >> k) : 1u, h = (height >> k) ? (height >> k) : 1u,
				d = (depth >> k) ? (depth >> k) : 1u;
			const size_t slice_bytes = (size_t)w*h*16u;
			// the slice buffer is a context buffer like the staging buffers: owned through the same lease
			rc = lease.acquire();
			if (rc == CFHIP_OK)
				rc = reserve(ctx, &ctx->d_mip3d, &ctx->mip3d_cap, slice_bytes*pd);
			if (rc != CFHIP_OK)
				return rc;
			for (uint32_t i = 0; i < pd; ++i) {
				uint8_t* dst = static_cast<uint8_t*>(ctx->d_mip3d) + slice_bytes*i;
				if (w == pw && h == ph)    // Image::resize returns a copy (Image.cpp:1330-1334): an exact Box identity
					HIP_TRY(ctx, cfhip_launch_mip_resize(prev + prev_slice*i, prev_type, prev_pitch, pw, ph, dst, w, h,
						CFHIP_FILTER_BOX, 0, stream));
				else {
					rc = mip_level_2d(ctx, lease, prev + prev_slice*i, prev_type, prev_pitch, pw, ph, dst, w, h, filter, srgb);
					if (rc != CFHIP_OK)
						return rc;
				}
			}
			HIP_TRY(ctx, cfhip_launch_mip_depth(ctx->d_mip3d, pd, w*h, dst_levels[k - 1], d,
				(filter & 0xFF) == CFHIP_FILTER_BOX ? 1 : 0, srgb, stream));
			prev = static_cast<const uint8_t*>(dst_levels[k - 1]);
			prev_type = CFHIP_PIXEL_RGBA32F;
			prev_pitch = (size_t)w*16u;
			prev_slice = slice_bytes;
			pw = w; ph = h; pd = d;
		}
		return lease.done(!stream_);
	});
}

int cfhip_decoded_layout(int format, int type, int* layout, int* texel_bytes)
{
	int l, tb;
	if (!decoded_layout(format, type, &l, &tb))
		return CFHIP_E_UNSUPPORTED;
	if (layout) *layout = l;
	if (texel_bytes) *texel_bytes = tb;
	return CFHIP_OK;
}

int cfhip_decode(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes, uint32_t width,
	uint32_t height, void* out, size_t out_capacity, uint64_t* error_blocks)
{
	return guarded(ctx, "decode", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		DecodeGeom g;
		int rc = decode_check(ctx, "decode", format, type, blocks, width, height, false, &g);
		if (rc != CFHIP_OK)
			return rc;
		if (!out)
			return fail(ctx, CFHIP_E_INVALID, "decode: out is NULL");
		if (blocks_bytes < g.payload_bytes)
			return fail(ctx, CFHIP_E_INVALID, "decode: blocks_bytes %zu < %zu for %ux%u", blocks_bytes, g.payload_bytes,
				width, height);
		const size_t out_bytes = (size_t)width*height*(size_t)g.texel_bytes;
		if (out_capacity < out_bytes)
			return fail(ctx, CFHIP_E_CAPACITY, "decode: out_capacity %zu < %zu", out_capacity, out_bytes);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payload; d_out: the texels, then the error-block counter
		const size_t cnt_off = (out_bytes + 15u) & ~(size_t)15u;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, g.payload_bytes);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, cnt_off + 8u);
		if (rc != CFHIP_OK)
			return rc;
		unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(ctx->d_out) + cnt_off);
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_src, blocks, g.payload_bytes, hipMemcpyHostToDevice, stream));
		HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, 8, stream));
		rc = decode_launch(ctx, format, type, g, ctx->d_src, ctx->d_out, (size_t)width*(size_t)g.texel_bytes, nullptr, 0,
			width, height, d_cnt, false, stream);
		if (rc != CFHIP_OK)
			return rc;
		unsigned long long count = 0;
		HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_out, out_bytes, hipMemcpyDeviceToHost, stream));
		HIP_TRY(ctx, hipMemcpyAsync(&count, d_cnt, 8, hipMemcpyDeviceToHost, stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		if (error_blocks)
			*error_blocks = (uint64_t)count;
		return CFHIP_OK;
	});
}

int cfhip_decode_device(cfhip_ctx* ctx, int format, int type, const void* blocks, uint32_t width, uint32_t height,
	void* out, size_t out_pitch_bytes, uint64_t* error_blocks_device, void* stream_)
{
	return guarded(ctx, "decode_device", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		DecodeGeom g;
		int rc = decode_check(ctx, "decode_device", format, type, blocks, width, height, false, &g);
		if (rc != CFHIP_OK)
			return rc;
		if (!out)
			return fail(ctx, CFHIP_E_INVALID, "decode_device: out is NULL");
		if (out_pitch_bytes < (size_t)width*(size_t)g.texel_bytes)
			return fail(ctx, CFHIP_E_INVALID, "decode_device: out pitch %zu < %zu", out_pitch_bytes,
				(size_t)width*(size_t)g.texel_bytes);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		// no staging buffer is touched: the lease only carries the synchronisation rule of the stream
		StagingLease lease(ctx, call_stream(ctx, stream_));
		unsigned long long* cnt = reinterpret_cast<unsigned long long*>(error_blocks_device);
		if (cnt)
			HIP_TRY(ctx, hipMemsetAsync(cnt, 0, 8, lease.stream));
		rc = decode_launch(ctx, format, type, g, blocks, out, out_pitch_bytes, nullptr, 0, width, height, cnt, false,
			lease.stream);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

// ---- batched decode (csrc/decode.hip: cfhip_decode_batch_kernel, cfhip_decode_batch_astc_kernel) -------------
// What a (layout, out_pixel) pair stores: false where the table of include/cuttlefish_hip.h says unsupported.
// *kind: the CFDEC_OUT_* value of the launch (a pixel type that equals the native layout is the native launch).
static bool decode_out_kind(int layout, int native_tb, int out_pixel, int* kind, int* out_tb)
{
	const bool u8 = layout == CFHIP_LAYOUT_RGBA8 || layout == CFHIP_LAYOUT_R8 || layout == CFHIP_LAYOUT_RG8;
	switch (out_pixel) {
		case CFHIP_DECODE_NATIVE: *kind = CFDEC_OUT_NATIVE; *out_tb = native_tb; return true;
		case CFHIP_PIXEL_RGBA8:
			if (!u8) return false;
			*kind = layout == CFHIP_LAYOUT_RGBA8 ? CFDEC_OUT_NATIVE : CFDEC_OUT_RGBA8; *out_tb = 4; return true;
		case CFHIP_PIXEL_RGBA16F:
			if (layout != CFHIP_LAYOUT_RGBA16F) return false;
			*kind = CFDEC_OUT_NATIVE; *out_tb = 8; return true;
		case CFHIP_PIXEL_RGBA32F: *kind = CFDEC_OUT_RGBA32F; *out_tb = 16; return true;
		default: return false;
	}
}

int cfhip_decode_out_supported(int format, int type, int out_pixel)
{
	int l, tb, kind, otb;
	return decoded_layout(format, type, &l, &tb) && decode_out_kind(l, tb, out_pixel, &kind, &otb) ? 1 : 0;
}

struct DecodeBatchPlan {
	int kind, out_tb, bw, bh, bb;
	std::vector<cfdec_batch_entry> entries;   // blocks / out still the caller's pointers
	std::vector<size_t> payload, span;        // payload bytes; bytes from out to the end of the last row
	uint32_t total_wg;
};

// Every check of a batched decode, made before the context is touched (so that they need no device): the pair,
// the output, the table and every surface.  ctx may be NULL here; the caller rejects that afterwards.
static int decode_batch_check(cfhip_ctx* ctx, const char* what, int format, int type, int out_pixel,
	const cfhip_decode_surface* s, size_t n, bool host, DecodeBatchPlan* p)
{
	int layout, tb;
	if (!decoded_layout(format, type, &layout, &tb))
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: (format %d, type %d) has no decoded layout", what, format, type);
	if (!decode_out_kind(layout, tb, out_pixel, &p->kind, &p->out_tb))
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: output pixel type %d is not offered for (format %d, type %d)", what,
			out_pixel, format, type);
	if (n && !s)
		return fail(ctx, CFHIP_E_INVALID, "%s: surfaces is NULL", what);
	if (n > 0xFFFFFFu)
		return fail(ctx, CFHIP_E_INVALID, "%s: too many surfaces (%zu)", what, n);
	block_dims(format, &p->bw, &p->bh);
	p->bb = block_bytes(format);
	const bool astc = format >= CFHIP_FORMAT_ASTC_4x4;
	p->entries.resize(n);
	p->payload.resize(n);
	p->span.resize(n);
	uint64_t wg = 0;
	for (size_t i = 0; i < n; ++i) {
		if (!s[i].blocks || !s[i].out)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: blocks or out is NULL", what, i);
		if (!s[i].width || !s[i].height)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu is empty (%ux%u)", what, i, s[i].width, s[i].height);
		const size_t row = (size_t)s[i].width*(size_t)p->out_tb;
		if (s[i].out_pitch_bytes < row)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: out pitch %zu < %zu", what, i, s[i].out_pitch_bytes, row);
		cfdec_batch_entry& e = p->entries[i];
		e.blocks = static_cast<const uint8_t*>(s[i].blocks);
		e.out = static_cast<uint8_t*>(s[i].out);
		e.out_pitch = s[i].out_pitch_bytes;
		e.width = s[i].width; e.height = s[i].height;
		e.bx = (e.width + (uint32_t)p->bw - 1)/(uint32_t)p->bw;
		e.by = (e.height + (uint32_t)p->bh - 1)/(uint32_t)p->bh;
		p->payload[i] = (size_t)e.bx*e.by*(size_t)p->bb;
		p->span[i] = (size_t)(e.height - 1)*s[i].out_pitch_bytes + row;
		if (host && s[i].blocks_bytes < p->payload[i])
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: blocks_bytes %zu < %zu", what, i, s[i].blocks_bytes,
				p->payload[i]);
		if (host && s[i].out_capacity < p->span[i])
			return fail(ctx, CFHIP_E_CAPACITY, "%s: surface %zu: out_capacity %zu < %zu", what, i, s[i].out_capacity,
				p->span[i]);
		e.wgx = astc ? (e.bx + CFDEC_ASTC_RUN - 1)/CFDEC_ASTC_RUN : 0;
		e.wg_begin = (uint32_t)wg;
		wg += astc ? (uint64_t)e.wgx*e.by : ((uint64_t)e.bx*e.by + CFDEC_WG - 1)/CFDEC_WG;
		if (wg > 0x7FFFFFFFull)
			return fail(ctx, CFHIP_E_INVALID, "%s: the surfaces are too large for one launch", what);
	}
	p->total_wg = (uint32_t)wg;
	return CFHIP_OK;
}

// the surface table into staging and the one launch of the call; the entries hold device pointers by now
static int decode_batch_launch(cfhip_ctx* ctx, StagingLease& lease, int format, int type, DecodeBatchPlan& p,
	unsigned long long* d_errors)
{
	const hipStream_t stream = lease.stream;
	begin_call(ctx, stream, format >= CFHIP_FORMAT_ASTC_4x4 ? "cfhip_decode_batch_astc_kernel" : "cfhip_decode_batch_kernel");
	for (cfdec_batch_entry& e : p.entries) {
		e.out_vec = ((uintptr_t)e.out % 16 == 0 && e.out_pitch % 16 == 0) ? 1 : 0;
		e.blk_vec = ((uintptr_t)e.blocks % (uintptr_t)p.bb == 0) ? 1 : 0;
	}
	const size_t bytes = p.entries.size()*sizeof(cfdec_batch_entry);
	int rc = lease.acquire();
	if (rc == CFHIP_OK)
		rc = reserve(ctx, &ctx->d_batch, &ctx->batch_cap, bytes);
	if (rc != CFHIP_OK)
		return rc;
	// pageable source: the runtime stages the copy before returning, so the plan may die
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, p.entries.data(), bytes, hipMemcpyHostToDevice, stream));
	if (d_errors)
		HIP_TRY(ctx, hipMemsetAsync(d_errors, 0, 8*p.entries.size(), stream));
	return timed(ctx, stream, "decode_batch", [&] {
		return cfhip_launch_decode_batch(format, type, p.kind, static_cast<const cfdec_batch_entry*>(ctx->d_batch),
			(uint32_t)p.entries.size(), p.total_wg, p.bw, p.bh, d_errors, stream);
	});
}

int cfhip_decode_batch(cfhip_ctx* ctx, int format, int type, int out_pixel, const cfhip_decode_surface* surfaces,
	size_t n, uint64_t* error_blocks)
{
	return guarded(ctx, "decode_batch", [&]() -> int {
		DecodeBatchPlan p;
		int rc = decode_batch_check(ctx, "decode_batch", format, type, out_pixel, surfaces, n, true, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		if (!n)
			return CFHIP_OK;
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payloads, a run of surfaces whose blocks are consecutive in host memory as one copy.  d_out: the
		// texels, a run of tightly pitched surfaces whose outputs are consecutive in host memory as one copy back (a
		// pitched output has rows of its own on the device and comes back as a 2-D copy); then the error counters.
		struct Run { size_t first, last, dev, bytes; };
		std::vector<Run> up, down;
		std::vector<size_t> src_off(n), out_off(n);
		size_t so = 0, oo = 0;
		for (size_t i = 0; i < n; ++i) {
			const uint8_t* b = static_cast<const uint8_t*>(surfaces[i].blocks);
			if (i && b == static_cast<const uint8_t*>(surfaces[i - 1].blocks) + p.payload[i - 1]) {
				src_off[i] = src_off[i - 1] + p.payload[i - 1];
				up.back().last = i;
				up.back().bytes += p.payload[i];
			} else {
				so = (so + 255) & ~(size_t)255;
				src_off[i] = so;
				up.push_back({i, i, so, p.payload[i]});
			}
			so = src_off[i] + p.payload[i];
			const bool tight = surfaces[i].out_pitch_bytes == (size_t)surfaces[i].width*(size_t)p.out_tb;
			const bool prev_tight = i && surfaces[i - 1].out_pitch_bytes == (size_t)surfaces[i - 1].width*(size_t)p.out_tb;
			if (tight && prev_tight && static_cast<uint8_t*>(surfaces[i].out) == static_cast<uint8_t*>(surfaces[i - 1].out) + p.span[i - 1]) {
				out_off[i] = out_off[i - 1] + p.span[i - 1];
				down.back().last = i;
				down.back().bytes += p.span[i];
			} else {
				oo = (oo + 255) & ~(size_t)255;
				out_off[i] = oo;
				down.push_back({i, i, oo, p.span[i]});
			}
			// on the device every surface is tightly pitched
			oo = out_off[i] + (size_t)surfaces[i].width*(size_t)p.out_tb*surfaces[i].height;
		}
		const size_t cnt_off = (oo + 255) & ~(size_t)255;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, so);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, cnt_off + 8*n);
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d_src = static_cast<uint8_t*>(ctx->d_src);
		uint8_t* d_out = static_cast<uint8_t*>(ctx->d_out);
		for (const Run& r : up)
			HIP_TRY(ctx, hipMemcpyAsync(d_src + r.dev, surfaces[r.first].blocks, r.bytes, hipMemcpyHostToDevice, stream));
		for (size_t i = 0; i < n; ++i) {
			p.entries[i].blocks = d_src + src_off[i];
			p.entries[i].out = d_out + out_off[i];
			p.entries[i].out_pitch = (size_t)surfaces[i].width*(size_t)p.out_tb;
		}
		unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(d_out + cnt_off);
		rc = decode_batch_launch(ctx, lease, format, type, p, d_cnt);
		if (rc != CFHIP_OK)
			return rc;
		for (const Run& r : down) {
			const cfhip_decode_surface& s = surfaces[r.first];
			const size_t row = (size_t)s.width*(size_t)p.out_tb;
			if (s.out_pitch_bytes == row)
				HIP_TRY(ctx, hipMemcpyAsync(s.out, d_out + r.dev, r.bytes, hipMemcpyDeviceToHost, stream));
			else
				HIP_TRY(ctx, hipMemcpy2DAsync(s.out, s.out_pitch_bytes, d_out + r.dev, row, row, s.height,
					hipMemcpyDeviceToHost, stream));
		}
		std::vector<unsigned long long> counts(n, 0);
		HIP_TRY(ctx, hipMemcpyAsync(counts.data(), d_cnt, 8*n, hipMemcpyDeviceToHost, stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		if (error_blocks)
			for (size_t i = 0; i < n; ++i)
				error_blocks[i] = (uint64_t)counts[i];
		return CFHIP_OK;
	});
}

int cfhip_decode_batch_device(cfhip_ctx* ctx, int format, int type, int out_pixel,
	const cfhip_decode_surface* surfaces, size_t n, uint64_t* error_blocks_device, void* stream_)
{
	return guarded(ctx, "decode_batch_device", [&]() -> int {
		DecodeBatchPlan p;
		int rc = decode_batch_check(ctx, "decode_batch_device", format, type, out_pixel, surfaces, n, false, &p);
		if (rc != CFHIP_OK)
			return rc;
		if ((uintptr_t)error_blocks_device % 8)
			return fail(ctx, CFHIP_E_INVALID, "decode_batch_device: error_blocks_device must be 8-byte aligned");
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		if (!n)
			return CFHIP_OK;
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		rc = decode_batch_launch(ctx, lease, format, type, p, reinterpret_cast<unsigned long long*>(error_blocks_device));
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

int cfhip_decode_sse(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes, uint32_t width,
	uint32_t height, const void* ref_rgba8, size_t ref_pitch_bytes, uint64_t sse[4])
{
	return guarded(ctx, "decode_sse", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		DecodeGeom g;
		int rc = decode_check(ctx, "decode_sse", format, type, blocks, width, height, true, &g);
		if (rc != CFHIP_OK)
			return rc;
		if (!ref_rgba8 || !sse)
			return fail(ctx, CFHIP_E_INVALID, "decode_sse: NULL reference or result");
		if (blocks_bytes < g.payload_bytes)
			return fail(ctx, CFHIP_E_INVALID, "decode_sse: blocks_bytes %zu < %zu for %ux%u", blocks_bytes,
				g.payload_bytes, width, height);
		const size_t row = (size_t)width*4u;
		if (ref_pitch_bytes < row)
			return fail(ctx, CFHIP_E_INVALID, "decode_sse: reference pitch %zu < %zu", ref_pitch_bytes, row);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payload; d_out: the reference, tightly packed, then the four sums
		const size_t sum_off = (row*height + 15u) & ~(size_t)15u;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, g.payload_bytes);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, sum_off + 32u);
		if (rc != CFHIP_OK)
			return rc;
		unsigned long long* d_sum = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(ctx->d_out) + sum_off);
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_src, blocks, g.payload_bytes, hipMemcpyHostToDevice, stream));
		HIP_TRY(ctx, hipMemcpy2DAsync(ctx->d_out, row, ref_rgba8, ref_pitch_bytes, row, height, hipMemcpyHostToDevice,
			stream));
		HIP_TRY(ctx, hipMemsetAsync(d_sum, 0, 32, stream));
		rc = decode_launch(ctx, format, type, g, ctx->d_src, nullptr, 0, ctx->d_out, row, width, height, d_sum, true,
			stream);
		if (rc != CFHIP_OK)
			return rc;
		unsigned long long sums[4] = {0, 0, 0, 0};
		HIP_TRY(ctx, hipMemcpyAsync(sums, d_sum, 32, hipMemcpyDeviceToHost, stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		for (int c = 0; c < 4; ++c)
			sse[c] = (uint64_t)sums[c];
		return CFHIP_OK;
	});
}

int cfhip_decode_sse_device(cfhip_ctx* ctx, int format, int type, const void* blocks, uint32_t width,
	uint32_t height, const void* ref_rgba8, size_t ref_pitch_bytes, uint64_t* sse_device, void* stream_)
{
	return guarded(ctx, "decode_sse_device", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		DecodeGeom g;
		int rc = decode_check(ctx, "decode_sse_device", format, type, blocks, width, height, true, &g);
		if (rc != CFHIP_OK)
			return rc;
		if (!ref_rgba8 || !sse_device)
			return fail(ctx, CFHIP_E_INVALID, "decode_sse_device: NULL reference or result");
		if (ref_pitch_bytes < (size_t)width*4u)
			return fail(ctx, CFHIP_E_INVALID, "decode_sse_device: reference pitch %zu < %zu", ref_pitch_bytes,
				(size_t)width*4u);
		// the kernels add to the four sums with 64-bit atomics
		if ((uintptr_t)sse_device % 8u != 0)
			return fail(ctx, CFHIP_E_INVALID, "decode_sse_device: sse_device must be 8-byte aligned");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		unsigned long long* sum = reinterpret_cast<unsigned long long*>(sse_device);
		HIP_TRY(ctx, hipMemsetAsync(sum, 0, 32, lease.stream));
		rc = decode_launch(ctx, format, type, g, blocks, nullptr, 0, ref_rgba8, ref_pitch_bytes, width, height, sum, true,
			lease.stream);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

int cfhip_compare(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes, uint32_t width,
	uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch_bytes, const uint8_t mask_rgba[4],
	unsigned flags, cfhip_compare_result* result, float* block_errors, size_t block_errors_capacity)
{
	return guarded(ctx, "compare", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		CompareGeom c;
		int rc = compare_check(ctx, "compare", format, type, blocks, width, height, ref, ref_pixel_type, ref_pitch_bytes,
			mask_rgba, flags, result, block_errors, block_errors_capacity, &c);
		if (rc != CFHIP_OK)
			return rc;
		if (blocks_bytes < c.g.payload_bytes)
			return fail(ctx, CFHIP_E_INVALID, "compare: blocks_bytes %zu < %zu for %ux%u", blocks_bytes,
				c.g.payload_bytes, width, height);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payload; d_out: the reference, tightly packed, the scratch, the result, the block map
		const size_t row = (size_t)width*(size_t)c.ref_bytes;
		const size_t scr_off = align16(row*height), res_off = align16(scr_off + c.scratch_bytes);
		const size_t map_off = align16(res_off + sizeof(cfhip_compare_result));
		const size_t map_bytes = block_errors ? (size_t)c.g.bx*c.g.by*sizeof(float) : 0;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, c.g.payload_bytes);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, map_off + map_bytes);
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d = static_cast<uint8_t*>(ctx->d_out);
		cfhip_compare_result* d_res = reinterpret_cast<cfhip_compare_result*>(d + res_off);
		float* d_map = block_errors ? reinterpret_cast<float*>(d + map_off) : nullptr;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_src, blocks, c.g.payload_bytes, hipMemcpyHostToDevice, stream));
		HIP_TRY(ctx, hipMemcpy2DAsync(d, row, ref, ref_pitch_bytes, row, height, hipMemcpyHostToDevice, stream));
		rc = compare_enqueue(ctx, format, type, c, ctx->d_src, d, ref_pixel_type, row, width, height, d + scr_off, d_res,
			d_map, stream);
		if (rc != CFHIP_OK)
			return rc;
		cfhip_compare_result res;
		HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, stream));
		if (d_map)
			HIP_TRY(ctx, hipMemcpyAsync(block_errors, d_map, map_bytes, hipMemcpyDeviceToHost, stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		*result = res;
		return CFHIP_OK;
	});
}

int cfhip_compare_device(cfhip_ctx* ctx, int format, int type, const void* blocks, uint32_t width, uint32_t height,
	const void* ref, int ref_pixel_type, size_t ref_pitch_bytes, const uint8_t mask_rgba[4], unsigned flags,
	cfhip_compare_result* result_device, float* block_errors_device, size_t block_errors_capacity, void* stream_)
{
	return guarded(ctx, "compare_device", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		CompareGeom c;
		int rc = compare_check(ctx, "compare_device", format, type, blocks, width, height, ref, ref_pixel_type,
			ref_pitch_bytes, mask_rgba, flags, result_device, block_errors_device, block_errors_capacity, &c);
		if (rc != CFHIP_OK)
			return rc;
		// the kernels read reference texels with one aligned load each and store doubles / floats to the outputs
		const size_t rb = (size_t)c.ref_bytes;
		if ((uintptr_t)ref % rb != 0 || ref_pitch_bytes % rb != 0)
			return fail(ctx, CFHIP_E_INVALID, "compare_device: reference and its pitch must be %zu-byte aligned", rb);
		if ((uintptr_t)result_device % 8u != 0 || (uintptr_t)block_errors_device % 4u != 0)
			return fail(ctx, CFHIP_E_INVALID, "compare_device: misaligned result or block_errors");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		// the partials (and the SSIM pass's decoded surface) live in d_out: the lease orders them across streams
		StagingLease lease(ctx, call_stream(ctx, stream_));
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, c.scratch_bytes);
		if (rc != CFHIP_OK)
			return rc;
		rc = compare_enqueue(ctx, format, type, c, blocks, ref, ref_pixel_type, ref_pitch_bytes, width, height,
			static_cast<uint8_t*>(ctx->d_out), result_device, block_errors_device, lease.stream);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

// ---- batched compare (csrc/compare.hip: the cfhip_compare_batch_* kernels; csrc/compare_batch.h) -------------
// What one batched compare runs and where its device scratch lies: the decoded surfaces of the SSIM pass (each
// 16-byte aligned, only those with a valid window), then the Pass A partials of every workgroup of the call, then
// the SSIM partials of every tile.  The scratch grows with the sum over the surfaces and is not capped.
struct CompareBatchPlan {
	int layout, texel_bytes, ref_bytes, bw, bh, bb;
	unsigned cmask;
	bool hdr, ssim;                           // ssim: the SSIM pass runs (some surface has a valid window)
	std::vector<cmp_batch_entry> entries;     // blocks / ref / block_errors still the caller's pointers
	std::vector<size_t> payload;              // payload bytes
	uint32_t total_wg, total_tiles;
	size_t pa_off, pb_off, scratch_bytes;
};

// Every check of a batched compare, made before the context is touched (so that they need no device): the pair,
// the table and every surface, each by compare_check, the rules of the per-surface entries.  ctx may be NULL here;
// the caller rejects that afterwards.
static int compare_batch_check(cfhip_ctx* ctx, const char* what, int format, int type, const cfhip_compare_surface* s,
	size_t n, int ref_pixel_type, const uint8_t* mask, unsigned flags, const void* results, bool host,
	CompareBatchPlan* p)
{
	if (!decoded_layout(format, type, &p->layout, &p->texel_bytes))
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: (format %d, type %d) has no decoded layout", what, format, type);
	p->total_wg = p->total_tiles = 0;
	if (!n)
		return CFHIP_OK;
	if (!s || !results)
		return fail(ctx, CFHIP_E_INVALID, "%s: surfaces or results is NULL", what);
	if (n > 0xFFFFFFu)
		return fail(ctx, CFHIP_E_INVALID, "%s: too many surfaces (%zu)", what, n);
	if ((uintptr_t)results % 8u != 0)
		return fail(ctx, CFHIP_E_INVALID, "%s: results must be 8-byte aligned", what);
	const bool astc = format >= CFHIP_FORMAT_ASTC_4x4;
	p->entries.resize(n);
	p->payload.resize(n);
	uint64_t wg = 0, tiles = 0;
	size_t dec = 0;
	for (size_t i = 0; i < n; ++i) {
		char who[64];
		snprintf(who, sizeof(who), "%s: surface %zu", what, i);
		CompareGeom c;
		const int rc = compare_check(ctx, who, format, type, s[i].blocks, s[i].width, s[i].height, s[i].ref,
			ref_pixel_type, s[i].ref_pitch_bytes, mask, flags, results, s[i].block_errors, s[i].block_errors_capacity, &c);
		if (rc != CFHIP_OK)
			return rc;
		if (host && s[i].blocks_bytes < c.g.payload_bytes)
			return fail(ctx, CFHIP_E_INVALID, "%s: blocks_bytes %zu < %zu for %ux%u", who, s[i].blocks_bytes,
				c.g.payload_bytes, s[i].width, s[i].height);
		if (!host) {
			// the kernels read reference texels with one aligned load each and store floats to the maps
			const size_t rb = (size_t)c.ref_bytes;
			if ((uintptr_t)s[i].ref % rb != 0 || s[i].ref_pitch_bytes % rb != 0)
				return fail(ctx, CFHIP_E_INVALID, "%s: reference and its pitch must be %zu-byte aligned", who, rb);
			if ((uintptr_t)s[i].block_errors % 4u != 0)
				return fail(ctx, CFHIP_E_INVALID, "%s: misaligned block_errors", who);
		}
		if (!i) {
			p->ref_bytes = c.ref_bytes; p->cmask = c.cmask; p->hdr = c.hdr;
			p->bw = c.g.bw; p->bh = c.g.bh; p->bb = c.g.bb;
		}
		cmp_batch_entry& e = p->entries[i];
		e.blocks = static_cast<const uint8_t*>(s[i].blocks);
		e.ref = static_cast<const uint8_t*>(s[i].ref);
		e.ref_pitch = s[i].ref_pitch_bytes;
		e.block_errors = s[i].block_errors;
		e.width = s[i].width; e.height = s[i].height; e.bx = c.g.bx; e.by = c.g.by;
		e.wgx = astc ? (e.bx + 63u)/64u : 0;
		e.wg_begin = (uint32_t)wg;
		e.na = (uint32_t)c.na;
		e.tile_begin = (uint32_t)tiles;
		e.tiles_x = c.ssim ? (e.width - 10u + 15u)/16u : 0;
		e.nb = (uint32_t)c.nb;
		e.windows = c.windows;
		e.dec_off = dec;
		e.blk_vec = 0;
		p->payload[i] = c.g.payload_bytes;
		wg += c.na;
		tiles += c.nb;
		if (c.ssim)
			dec = align16(dec + (size_t)e.width*e.height*(size_t)p->texel_bytes);
		if (c.na > 0x7FFFFFFFull || wg > 0x7FFFFFFFull || tiles > 0x7FFFFFFFull)
			return fail(ctx, CFHIP_E_INVALID, "%s: the surfaces are too large for one launch", what);
	}
	p->total_wg = (uint32_t)wg;
	p->total_tiles = (uint32_t)tiles;
	p->ssim = tiles > 0;
	p->pa_off = align16(dec);
	p->pb_off = p->pa_off + (size_t)wg*16u*sizeof(double);
	p->scratch_bytes = p->pb_off + (size_t)tiles*4u*sizeof(double);
	return CFHIP_OK;
}

// the surface tables into staging and the two (without an SSIM pass) or four launches of the call, each timed as
// every encode launch is; the entries hold device pointers by now
static int compare_batch_launch(cfhip_ctx* ctx, StagingLease& lease, int format, int type, int ref_pixel_type,
	CompareBatchPlan& p, uint8_t* scratch, cfhip_compare_result* results)
{
	const hipStream_t stream = lease.stream;
	begin_call(ctx, stream, format >= CFHIP_FORMAT_ASTC_4x4 ? "cfhip_compare_batch_astc_kernel" : "cfhip_compare_batch_block_kernel");
	const size_t n = p.entries.size();
	// the compare table, then the decode table of the surfaces the SSIM pass covers (the decoders' workgroup shapes
	// are Pass A's: 256 blocks, or a run of 64 ASTC blocks)
	std::vector<cfdec_batch_entry> dec;
	uint32_t dec_wg = 0;
	for (cmp_batch_entry& e : p.entries) {
		e.blk_vec = ((uintptr_t)e.blocks % (uintptr_t)p.bb == 0) ? 1 : 0;
		if (!e.nb)
			continue;
		cfdec_batch_entry d;
		d.blocks = e.blocks;
		d.out = scratch + e.dec_off;
		d.out_pitch = (unsigned long long)e.width*(unsigned)p.texel_bytes;
		d.width = e.width; d.height = e.height; d.bx = e.bx; d.by = e.by;
		d.wg_begin = dec_wg;
		d.wgx = e.wgx;
		d.out_vec = ((uintptr_t)d.out % 16 == 0 && d.out_pitch % 16 == 0) ? 1 : 0;
		d.blk_vec = e.blk_vec;
		dec_wg += e.na;
		dec.push_back(d);
	}
	const size_t cmp_bytes = n*sizeof(cmp_batch_entry), dec_off = align16(cmp_bytes);
	std::vector<uint8_t> tables(dec_off + dec.size()*sizeof(cfdec_batch_entry));
	memcpy(tables.data(), p.entries.data(), cmp_bytes);
	if (!dec.empty())
		memcpy(tables.data() + dec_off, dec.data(), dec.size()*sizeof(cfdec_batch_entry));
	int rc = lease.acquire();
	if (rc == CFHIP_OK)
		rc = reserve(ctx, &ctx->d_batch, &ctx->batch_cap, tables.size());
	if (rc != CFHIP_OK)
		return rc;
	// pageable source: the runtime stages the copy before returning, so the tables may die
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, tables.data(), tables.size(), hipMemcpyHostToDevice, stream));
	const cmp_batch_entry* d_cmp = static_cast<const cmp_batch_entry*>(ctx->d_batch);
	const cfdec_batch_entry* d_dec = reinterpret_cast<const cfdec_batch_entry*>(static_cast<uint8_t*>(ctx->d_batch) + dec_off);
	double* pa = reinterpret_cast<double*>(scratch + p.pa_off);
	double* pb = p.ssim ? reinterpret_cast<double*>(scratch + p.pb_off) : nullptr;
	const int steps = p.ssim ? 4 : 2;
	for (int step = 0; step < steps; ++step) {
		rc = timed(ctx, stream, "compare_batch", [&] {
			if (step == 0)
				return cfhip_launch_compare_batch(format, type, d_cmp, (uint32_t)n, p.total_wg, p.bw, p.bh, ref_pixel_type,
					p.cmask, pa, stream);
			if (step == steps - 1)
				return cfhip_launch_compare_batch_final(d_cmp, (uint32_t)n, pa, pb, p.cmask, p.hdr ? 1 : 0, results, stream);
			if (step == 1)
				return cfhip_launch_decode_batch(format, type, CFDEC_OUT_NATIVE, d_dec, (uint32_t)dec.size(), dec_wg, p.bw, p.bh,
					nullptr, stream);
			const int l = p.layout;
			const double range = (l == CFHIP_LAYOUT_R8_SNORM || l == CFHIP_LAYOUT_RG8_SNORM ||
				l == CFHIP_LAYOUT_R16_SNORM || l == CFHIP_LAYOUT_RG16_SNORM) ? 2.0 : 1.0;
			return cfhip_launch_ssim_batch(d_cmp, (uint32_t)n, p.total_tiles, scratch, l, ref_pixel_type, p.cmask,
				ssim_taps(), range, pb, stream);
		});
		if (rc != CFHIP_OK)
			return rc;
	}
	return CFHIP_OK;
}

int cfhip_compare_batch(cfhip_ctx* ctx, int format, int type, const cfhip_compare_surface* surfaces, size_t n,
	int ref_pixel_type, const uint8_t mask_rgba[4], unsigned flags, cfhip_compare_result* results)
{
	return guarded(ctx, "compare_batch", [&]() -> int {
		CompareBatchPlan p;
		int rc = compare_batch_check(ctx, "compare_batch", format, type, surfaces, n, ref_pixel_type, mask_rgba, flags,
			results, true, &p);
		if (rc != CFHIP_OK || !n)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payloads, a run of surfaces whose blocks are consecutive in host memory as one copy.  d_out: the
		// references, tightly pitched and packed without gaps (a texel keeps its alignment: every surface is a whole
		// number of texels), so that tight references that are consecutive in host memory are one copy too; then the
		// scratch, the n results and the error maps.
		struct Run { size_t first, dev, bytes; };
		std::vector<Run> up, refs;
		std::vector<size_t> src_off(n), ref_off(n), map_off(n);
		size_t so = 0, ro = 0;
		bool prev_tight = false;
		const uint8_t* prev_end = nullptr;
		for (size_t i = 0; i < n; ++i) {
			const uint8_t* b = static_cast<const uint8_t*>(surfaces[i].blocks);
			if (i && b == static_cast<const uint8_t*>(surfaces[i - 1].blocks) + p.payload[i - 1]) {
				src_off[i] = src_off[i - 1] + p.payload[i - 1];
				up.back().bytes += p.payload[i];
			} else {
				so = (so + 255) & ~(size_t)255;
				src_off[i] = so;
				up.push_back({i, so, p.payload[i]});
			}
			so = src_off[i] + p.payload[i];
			const size_t row = (size_t)surfaces[i].width*(size_t)p.ref_bytes, bytes = row*surfaces[i].height;
			const bool tight = surfaces[i].ref_pitch_bytes == row;
			ref_off[i] = ro;
			if (tight && prev_tight && static_cast<const uint8_t*>(surfaces[i].ref) == prev_end)
				refs.back().bytes += bytes;
			else
				refs.push_back({i, ro, bytes});
			prev_tight = tight;
			prev_end = static_cast<const uint8_t*>(surfaces[i].ref) + bytes;
			ro += bytes;
		}
		const size_t scr_off = align16(ro), res_off = align16(scr_off + p.scratch_bytes);
		size_t mo = align16(res_off + n*sizeof(cfhip_compare_result));
		for (size_t i = 0; i < n; ++i) {
			map_off[i] = mo;
			if (surfaces[i].block_errors)
				mo = align16(mo + (size_t)p.entries[i].bx*p.entries[i].by*sizeof(float));
		}
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, so);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, mo);
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d_src = static_cast<uint8_t*>(ctx->d_src);
		uint8_t* d = static_cast<uint8_t*>(ctx->d_out);
		for (const Run& r : up)
			HIP_TRY(ctx, hipMemcpyAsync(d_src + r.dev, surfaces[r.first].blocks, r.bytes, hipMemcpyHostToDevice, stream));
		for (const Run& r : refs) {
			const cfhip_compare_surface& s = surfaces[r.first];
			const size_t row = (size_t)s.width*(size_t)p.ref_bytes;
			if (s.ref_pitch_bytes == row)
				HIP_TRY(ctx, hipMemcpyAsync(d + r.dev, s.ref, r.bytes, hipMemcpyHostToDevice, stream));
			else
				HIP_TRY(ctx, hipMemcpy2DAsync(d + r.dev, row, s.ref, s.ref_pitch_bytes, row, s.height, hipMemcpyHostToDevice,
					stream));
		}
		for (size_t i = 0; i < n; ++i) {
			cmp_batch_entry& e = p.entries[i];
			e.blocks = d_src + src_off[i];
			e.ref = d + ref_off[i];
			e.ref_pitch = (unsigned long long)e.width*(unsigned)p.ref_bytes;
			e.block_errors = surfaces[i].block_errors ? reinterpret_cast<float*>(d + map_off[i]) : nullptr;
		}
		cfhip_compare_result* d_res = reinterpret_cast<cfhip_compare_result*>(d + res_off);
		rc = compare_batch_launch(ctx, lease, format, type, ref_pixel_type, p, d + scr_off, d_res);
		if (rc != CFHIP_OK)
			return rc;
		std::vector<cfhip_compare_result> res(n);
		HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_res, n*sizeof(cfhip_compare_result), hipMemcpyDeviceToHost, stream));
		for (size_t i = 0; i < n; ++i)
			if (surfaces[i].block_errors)
				HIP_TRY(ctx, hipMemcpyAsync(surfaces[i].block_errors, d + map_off[i],
					(size_t)p.entries[i].bx*p.entries[i].by*sizeof(float), hipMemcpyDeviceToHost, stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		for (size_t i = 0; i < n; ++i)
			results[i] = res[i];
		return CFHIP_OK;
	});
}

int cfhip_compare_batch_device(cfhip_ctx* ctx, int format, int type, const cfhip_compare_surface* surfaces, size_t n,
	int ref_pixel_type, const uint8_t mask_rgba[4], unsigned flags, cfhip_compare_result* results_device, void* stream_)
{
	return guarded(ctx, "compare_batch_device", [&]() -> int {
		CompareBatchPlan p;
		int rc = compare_batch_check(ctx, "compare_batch_device", format, type, surfaces, n, ref_pixel_type, mask_rgba,
			flags, results_device, false, &p);
		if (rc != CFHIP_OK || !n)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		// the partials (and the SSIM pass's decoded surfaces) live in d_out, the tables in d_batch: the lease orders them
		// across streams
		StagingLease lease(ctx, call_stream(ctx, stream_));
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, p.scratch_bytes);
		if (rc != CFHIP_OK)
			return rc;
		rc = compare_batch_launch(ctx, lease, format, type, ref_pixel_type, p, static_cast<uint8_t*>(ctx->d_out),
			results_device);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

// ---- rate-distortion optimisation of BC1-5 / BC7 payloads (csrc/rdo.hip, csrc/rdo.h) ---------------------------
struct RdoPlan {
	int row;
	uint32_t lam16, cap;
	unsigned cmask;
	std::vector<cfrdo_entry> entries;         // blocks / out / pixels still the caller's pointers
	std::vector<size_t> payload, texel;       // payload bytes; bytes of a source texel
	uint32_t total_seg;
	bool row_above;                           // CFHIP_RDO_ROW_ABOVE: the 2-D kernel, one wavefront per tile
	uint32_t total_tile;
};

// Every check of an RDO call, made before the context is touched (so that they need no device).  ctx may be NULL
// here; the caller rejects that afterwards.  The parameters come as params (cfhip_rdo*) or as ex (cfhip_rdo_ex*).
static int rdo_check(cfhip_ctx* ctx, const char* what, int format, int type, const cfhip_rdo_surface* s, size_t n,
	const cfhip_rdo_params* params, const cfhip_rdo_ex_params* ex, const uint8_t* mask, const void* stats, bool host,
	RdoPlan* p)
{
	p->row = cfrdo_find_row(format, type);
	if (p->row < 0)
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: (format %d, type %d) is outside the RDO table", what, format, type);
	p->total_seg = p->total_tile = 0;
	p->row_above = false;
	if (!n)
		return CFHIP_OK;
	if (!s || !(params || ex) || !stats)
		return fail(ctx, CFHIP_E_INVALID, "%s: surfaces, params or stats is NULL", what);
	if (ex && ex->struct_size != sizeof(cfhip_rdo_ex_params))
		return fail(ctx, CFHIP_E_INVALID, "%s: struct_size %u is not %zu", what, ex->struct_size, sizeof(cfhip_rdo_ex_params));
	const float lambda = ex ? ex->lambda : params->lambda;
	if (!(lambda > 0.0f && lambda <= 1024.0f))
		return fail(ctx, CFHIP_E_INVALID, "%s: lambda %g is outside (0, 1024]", what, (double)lambda);
	uint32_t window = 32768u;
	if (ex) {
		if (ex->flags & ~CFHIP_RDO_ROW_ABOVE)
			return fail(ctx, CFHIP_E_INVALID, "%s: unknown flags 0x%x", what, ex->flags);
		if (ex->window_bytes && (ex->window_bytes < 64u || ex->window_bytes > (1u << 30)))
			return fail(ctx, CFHIP_E_INVALID, "%s: window_bytes %u is outside 64 .. 2^30", what, ex->window_bytes);
		if (ex->reserved[0] || ex->reserved[1] || ex->reserved[2])
			return fail(ctx, CFHIP_E_INVALID, "%s: reserved parameters must be 0", what);
		p->row_above = (ex->flags & CFHIP_RDO_ROW_ABOVE) != 0;
		if (ex->window_bytes)
			window = ex->window_bytes;
	} else if (params->reserved[0] || params->reserved[1])
		return fail(ctx, CFHIP_E_INVALID, "%s: reserved parameters must be 0", what);
	if (n > 0xFFFFFFu)
		return fail(ctx, CFHIP_E_INVALID, "%s: too many surfaces (%zu)", what, n);
	if ((uintptr_t)stats % 8u != 0)
		return fail(ctx, CFHIP_E_INVALID, "%s: stats must be 8-byte aligned", what);
	p->lam16 = (uint32_t)std::floor((double)lambda*16.0 + 0.5);
	p->cap = ex ? ex->max_sse_increase : params->max_sse_increase;
	unsigned m = 15u;
	if (mask)
		m = (mask[0] ? 1u : 0u) | (mask[1] ? 2u : 0u) | (mask[2] ? 4u : 0u) | (mask[3] ? 8u : 0u);
	const cfrdo_row& row = kCfrdoRows[p->row];
	p->cmask = row.channels & m;
	p->entries.resize(n);
	p->payload.resize(n);
	p->texel.resize(n);
	uint64_t segs = 0, tiles = 0;
	for (size_t i = 0; i < n; ++i) {
		if (!s[i].blocks || !s[i].out || !s[i].pixels)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: blocks, out or pixels is NULL", what, i);
		if (!s[i].width || !s[i].height)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: empty surface %ux%u", what, i, s[i].width, s[i].height);
		size_t tb;
		switch (s[i].pixel_type) {
			case CFHIP_PIXEL_RGBA8: tb = 4; break;
			case CFHIP_PIXEL_RGBA32F: tb = 16; break;
			case CFHIP_PIXEL_RGBA16F: tb = 8; break;
			default: return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: pixel type %d", what, i, s[i].pixel_type);
		}
		if (s[i].row_pitch_bytes < (size_t)s[i].width*tb)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: row pitch %zu < %zu", what, i, s[i].row_pitch_bytes,
				(size_t)s[i].width*tb);
		if (!host && ((uintptr_t)s[i].pixels % tb != 0 || s[i].row_pitch_bytes % tb != 0))
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: pixels and their pitch must be %zu-byte aligned", what, i, tb);
		const uint32_t bx = (s[i].width + 3u)/4u, by = (s[i].height + 3u)/4u;
		const size_t bytes = (size_t)bx*by*(size_t)row.block_bytes;
		if (host && s[i].blocks_bytes < bytes)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: blocks_bytes %zu < %zu for %ux%u", what, i,
				s[i].blocks_bytes, bytes, s[i].width, s[i].height);
		if (s[i].out_capacity < bytes)
			return fail(ctx, CFHIP_E_CAPACITY, "%s: surface %zu: out_capacity %zu < %zu", what, i, s[i].out_capacity, bytes);
		cfrdo_entry& e = p->entries[i];
		e.blocks = static_cast<const uint8_t*>(s[i].blocks);
		e.out = static_cast<uint8_t*>(s[i].out);
		e.pixels = static_cast<const uint8_t*>(s[i].pixels);
		e.pitch = s[i].row_pitch_bytes;
		e.width = s[i].width; e.height = s[i].height; e.bx = bx; e.by = by;
		e.seg_begin = (uint32_t)segs;
		e.segx = (bx + CFRDO_SEG - 1u)/CFRDO_SEG;
		e.pix = (uint32_t)s[i].pixel_type;
		e.vec = 0;
		p->payload[i] = bytes;
		p->texel[i] = tb;
		e.tile_begin = (uint32_t)tiles;
		e.up = p->row_above && ((uint64_t)bx + CFRDO_UP/2)*(uint64_t)row.block_bytes <= window ? 1u : 0u;
		segs += (uint64_t)e.segx*by;
		tiles += (uint64_t)e.segx*((by + CFRDO_TILE_ROWS - 1u)/CFRDO_TILE_ROWS);
		if (segs > 0x7FFFFFFFull)
			return fail(ctx, CFHIP_E_INVALID, "%s: the surfaces are too large for one launch", what);
	}
	p->total_seg = (uint32_t)segs;
	p->total_tile = (uint32_t)tiles;
	return CFHIP_OK;
}

static const char* rdo_kernel(const RdoPlan& p)
{
	return p.row_above ? "cfhip_rdo2d_kernel" : "cfhip_rdo_kernel";
}

// the surface table into staging, the counters cleared and the one launch of the call, timed as every encode launch
// is; the entries hold device pointers by now
// keep_events: a trial of cfhip_rdo_target, which began the call itself: the trial's pair joins those before it
static int rdo_launch(cfhip_ctx* ctx, StagingLease& lease, RdoPlan& p, cfhip_rdo_stats* stats, bool keep_events = false)
{
	static_assert(sizeof(cfhip_rdo_stats) == CFRDO_STATS*sizeof(unsigned long long), "the kernel's counters are the struct");
	const hipStream_t stream = lease.stream;
	if (!keep_events)
		begin_call(ctx, stream, rdo_kernel(p));
	else
		ctx->last_kernel = rdo_kernel(p);
	const size_t n = p.entries.size();
	const size_t bb = (size_t)kCfrdoRows[p.row].block_bytes;
	for (cfrdo_entry& e : p.entries)
		e.vec = ((uintptr_t)e.blocks % bb == 0 && (uintptr_t)e.out % bb == 0) ? 1 : 0;
	int rc = lease.acquire();
	if (rc == CFHIP_OK)
		rc = reserve(ctx, &ctx->d_batch, &ctx->batch_cap, n*sizeof(cfrdo_entry));
	if (rc != CFHIP_OK)
		return rc;
	// pageable source: the runtime stages the copy before returning, so the table may die
	HIP_TRY(ctx, hipMemcpyAsync(ctx->d_batch, p.entries.data(), n*sizeof(cfrdo_entry), hipMemcpyHostToDevice, stream));
	HIP_TRY(ctx, hipMemsetAsync(stats, 0, n*sizeof(cfhip_rdo_stats), stream));
	const cfrdo_entry* table = static_cast<const cfrdo_entry*>(ctx->d_batch);
	unsigned long long* counters = reinterpret_cast<unsigned long long*>(stats);
	return timed(ctx, stream, "rdo", [&] {
		return p.row_above
			? cfhip_launch_rdo2d(p.row, table, (uint32_t)n, p.total_tile, p.lam16, p.cap, p.cmask, counters, stream)
			: cfhip_launch_rdo(p.row, table, (uint32_t)n, p.total_seg, p.lam16, p.cap, p.cmask, counters, stream);
	});
}

int cfhip_rdo_supported(int format, int type)
{
	return cfrdo_find_row(format, type) >= 0 ? 1 : 0;
}

// cfhip_rdo and cfhip_rdo_ex: one of params and ex is the caller's
static int rdo_host(cfhip_ctx* ctx, const char* what, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_params* params, const cfhip_rdo_ex_params* ex, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats)
{
	return guarded(ctx, what, [&]() -> int {
		RdoPlan p;
		int rc = rdo_check(ctx, what, format, type, surfaces, n, params, ex, mask_rgba, stats, true, &p);
		if (rc != CFHIP_OK || !n)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payloads (optimised in place there), each 256-byte aligned; d_out: the sources, tightly pitched and
		// 16-byte aligned, then the counters
		std::vector<size_t> blk_off(n), pix_off(n);
		size_t so = 0, po = 0;
		for (size_t i = 0; i < n; ++i) {
			blk_off[i] = so;
			so = (so + p.payload[i] + 255u) & ~(size_t)255u;
			pix_off[i] = po;
			po = align16(po + (size_t)surfaces[i].width*p.texel[i]*surfaces[i].height);
		}
		const size_t stats_off = po;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, so);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, stats_off + n*sizeof(cfhip_rdo_stats));
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d_blk = static_cast<uint8_t*>(ctx->d_src);
		uint8_t* d = static_cast<uint8_t*>(ctx->d_out);
		for (size_t i = 0; i < n; ++i) {
			const cfhip_rdo_surface& s = surfaces[i];
			const size_t rowb = (size_t)s.width*p.texel[i];
			HIP_TRY(ctx, hipMemcpyAsync(d_blk + blk_off[i], s.blocks, p.payload[i], hipMemcpyHostToDevice, stream));
			if (s.row_pitch_bytes == rowb)
				HIP_TRY(ctx, hipMemcpyAsync(d + pix_off[i], s.pixels, rowb*s.height, hipMemcpyHostToDevice, stream));
			else
				HIP_TRY(ctx, hipMemcpy2DAsync(d + pix_off[i], rowb, s.pixels, s.row_pitch_bytes, rowb, s.height,
					hipMemcpyHostToDevice, stream));
			cfrdo_entry& e = p.entries[i];
			e.blocks = e.out = d_blk + blk_off[i];
			e.pixels = d + pix_off[i];
			e.pitch = rowb;
		}
		cfhip_rdo_stats* d_stats = reinterpret_cast<cfhip_rdo_stats*>(d + stats_off);
		rc = rdo_launch(ctx, lease, p, d_stats);
		if (rc != CFHIP_OK)
			return rc;
		std::vector<cfhip_rdo_stats> res(n);
		HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_stats, n*sizeof(cfhip_rdo_stats), hipMemcpyDeviceToHost, stream));
		for (size_t i = 0; i < n; ++i)
			HIP_TRY(ctx, hipMemcpyAsync(surfaces[i].out, d_blk + blk_off[i], p.payload[i], hipMemcpyDeviceToHost, stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		for (size_t i = 0; i < n; ++i)
			stats[i] = res[i];
		return CFHIP_OK;
	});
}

// cfhip_rdo_device and cfhip_rdo_ex_device
static int rdo_device(cfhip_ctx* ctx, const char* what, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_params* params, const cfhip_rdo_ex_params* ex, const uint8_t mask_rgba[4],
	cfhip_rdo_stats* stats_device, void* stream_)
{
	return guarded(ctx, what, [&]() -> int {
		RdoPlan p;
		int rc = rdo_check(ctx, what, format, type, surfaces, n, params, ex, mask_rgba, stats_device, false, &p);
		if (rc != CFHIP_OK || !n)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		// the surface table lives in d_batch: the lease orders it across streams
		StagingLease lease(ctx, call_stream(ctx, stream_));
		rc = rdo_launch(ctx, lease, p, stats_device);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

int cfhip_rdo(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats)
{
	return rdo_host(ctx, "rdo", format, type, surfaces, n, params, nullptr, mask_rgba, stats);
}

int cfhip_rdo_ex(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_ex_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats)
{
	return rdo_host(ctx, "rdo_ex", format, type, surfaces, n, nullptr, params, mask_rgba, stats);
}

int cfhip_rdo_device(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats_device, void* stream_)
{
	return rdo_device(ctx, "rdo_device", format, type, surfaces, n, params, nullptr, mask_rgba, stats_device, stream_);
}

int cfhip_rdo_ex_device(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_ex_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats_device, void* stream_)
{
	return rdo_device(ctx, "rdo_ex_device", format, type, surfaces, n, nullptr, params, mask_rgba, stats_device, stream_);
}

// ---- deflate-size estimate of payloads (csrc/lzsize.hip, csrc/lzsize.h) and RDO to a target ratio ----------------
struct LzPlan {
	std::vector<cfhip_lz_span> spans;         // the non-empty ones
	size_t total = 0;
};

// Every check of an estimator call, made before the context is touched.
static int lz_check(cfhip_ctx* ctx, const char* what, const cfhip_lz_span* spans, size_t n, const void* out, bool host,
	LzPlan* p)
{
	if (!out)
		return fail(ctx, CFHIP_E_INVALID, "%s: out is NULL", what);
	if (!host && (uintptr_t)out % 8u != 0)
		return fail(ctx, CFHIP_E_INVALID, "%s: out must be 8-byte aligned", what);
	if (n && !spans)
		return fail(ctx, CFHIP_E_INVALID, "%s: spans is NULL", what);
	for (size_t i = 0; i < n; ++i) {
		if (!spans[i].n)
			continue;
		if (!spans[i].bytes)
			return fail(ctx, CFHIP_E_INVALID, "%s: span %zu: bytes is NULL", what, i);
		if (spans[i].n >= ((size_t)1 << 31) || p->total + spans[i].n >= ((size_t)1 << 31))
			return fail(ctx, CFHIP_E_CAPACITY, "%s: the spans hold 2^31 bytes or more", what);
		p->total += spans[i].n;
		p->spans.push_back(spans[i]);
	}
	return CFHIP_OK;
}

// bytes [a, b) of the concatenated spans -> dst (device), on the stream
static int lz_gather(cfhip_ctx* ctx, const LzPlan& p, size_t a, size_t b, uint8_t* dst, hipMemcpyKind kind, hipStream_t stream)
{
	size_t at = 0;
	for (const cfhip_lz_span& s : p.spans) {
		const size_t lo = std::max(a, at), hi = std::min(b, at + s.n);
		if (lo < hi)
			HIP_TRY(ctx, hipMemcpyAsync(dst + (lo - a), static_cast<const uint8_t*>(s.bytes) + (lo - at), hi - lo, kind, stream));
		at += s.n;
		if (at >= b)
			break;
	}
	return CFHIP_OK;
}

static size_t lz_slice_of(const cfhip_ctx* ctx)
{
	size_t s = ctx->lz_slice ? ctx->lz_slice : (size_t)CFLZ_SLICE_DEFAULT;
	s = std::min(std::max(s, (size_t)CFLZ_COSTBLK), (size_t)1 << 30);     // before rounding: no overflow, never 0
	return (s + CFLZ_COSTBLK - 1u)/CFLZ_COSTBLK*CFLZ_COSTBLK;
}

// The slice of a stream of `total` bytes that is cut into whole `unit`s, and the scratch the sort of one slice (behind
// its window) takes.
static int lz_slice_plan(cfhip_ctx* ctx, size_t total, size_t unit, size_t* slice, size_t* sort_bytes)
{
	*slice = std::min(lz_slice_of(ctx), (total + unit - 1u)/unit*unit);
	HIP_TRY(ctx, cfhip_lz_sort_bytes(*slice + CFLZ_WINDOW, sort_bytes));
	return CFHIP_OK;
}

// The *_run routines below enqueue one codec's work on the lease's stream.  Their caller -- an entry point, its host
// wrapper, or the target search -- has acquired the lease, begun the call and, where the call keeps one, opened its
// stage log; the routines take their event pairs through take_event_pairs and know no family.

// The estimate of p's stream (total > 0) into six counters on the device: the stream in slices of whole cost blocks,
// each behind the W bytes before it.  out_device NULL: the scratch's own result slot, returned in *result.
static int lz_run(cfhip_ctx* ctx, StagingLease& lease, const LzPlan& p, hipMemcpyKind kind,
	unsigned long long* out_device, unsigned long long** result)
{
	const hipStream_t stream = lease.stream;
	size_t slice = 0, sort_bytes = 0;
	int rc = lz_slice_plan(ctx, p.total, CFLZ_COSTBLK, &slice, &sort_bytes);
	if (rc != CFHIP_OK)
		return rc;
	const cflz_layout lay = cflz_scratch(slice, sort_bytes);
	rc = reserve(ctx, &ctx->d_lz, &ctx->lz_cap, lay.total);
	if (rc != CFHIP_OK)
		return rc;
	uint8_t* base = static_cast<uint8_t*>(ctx->d_lz);
	unsigned long long* acc = reinterpret_cast<unsigned long long*>(base + lay.acc);
	if (!out_device)
		out_device = acc + 8;                 // the sums take 32 bytes of the 256 reserved
	if (result)
		*result = out_device;
	HIP_TRY(ctx, hipMemsetAsync(acc, 0, 4u*sizeof(unsigned long long), stream));
	for (size_t s0 = 0; s0 < p.total; s0 += slice) {
		const size_t s1 = std::min(p.total, s0 + slice);
		const size_t carry = s0 ? CFLZ_WINDOW : 0u;        // s0 >= one cost block > W
		rc = lz_gather(ctx, p, s0 - carry, s1, base + lay.bytes, kind, stream);
		if (rc != CFHIP_OK)
			return rc;
		hipEvent_t ev[2*CFLZ_STAGES];
		rc = take_event_pairs(ctx, ev, CFLZ_STAGES);
		if (rc != CFHIP_OK)
			return rc;
		const hipError_t e = cfhip_launch_lz_slice(base, &lay, sort_bytes, (uint32_t)carry, (uint32_t)(s1 - s0), ev, stream);
		if (e != hipSuccess)
			return fail(ctx, CFHIP_E_DEVICE, "lz_size launch: %s", hipGetErrorString(e));
	}
	const hipError_t e = cfhip_launch_lz_final(acc, (unsigned long long)p.total, out_device, stream);
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "lz_size launch: %s", hipGetErrorString(e));
	return CFHIP_OK;
}

int cfhip_lz_size(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, cfhip_lz_stats* out)
{
	static_assert(sizeof(cfhip_lz_stats) == 6*sizeof(unsigned long long), "the kernel's counters are the struct");
	return guarded(ctx, "lz_size", [&]() -> int {
		LzPlan p;
		int rc = lz_check(ctx, "lz_size", spans, n_spans, out, true, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!p.total) {
			memset(out, 0, sizeof(*out));
			return CFHIP_OK;
		}
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		begin_call(ctx, lease.stream, kLzSizeStages);
		unsigned long long* d_res = nullptr;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = lz_run(ctx, lease, p, hipMemcpyHostToDevice, nullptr, &d_res);
		if (rc != CFHIP_OK)
			return rc;
		cfhip_lz_stats res;
		HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, lease.stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		*out = res;
		return CFHIP_OK;
	});
}

int cfhip_lz_size_device(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, cfhip_lz_stats* out_device,
	void* stream_)
{
	return guarded(ctx, "lz_size_device", [&]() -> int {
		LzPlan p;
		int rc = lz_check(ctx, "lz_size_device", spans, n_spans, out_device, false, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		begin_call(ctx, lease.stream, kLzSizeStages);
		if (!p.total)
			HIP_TRY(ctx, hipMemsetAsync(out_device, 0, sizeof(cfhip_lz_stats), lease.stream));
		else {
			rc = lease.acquire();
			if (rc == CFHIP_OK)
				rc = lz_run(ctx, lease, p, hipMemcpyDeviceToDevice, reinterpret_cast<unsigned long long*>(out_device), nullptr);
			if (rc != CFHIP_OK)
				return rc;
		}
		return lease.done(!stream_);
	});
}

size_t cfhip_lz_slice_bytes(cfhip_ctx* ctx, size_t bytes)
{
	if (!ctx)
		return 0;
	std::lock_guard<std::mutex> guard(ctx->lock);
	const size_t before = lz_slice_of(ctx);
	ctx->lz_slice = bytes;
	return before;
}

int cfhip_lz_stage_ms(cfhip_ctx* ctx, float ms[CFLZ_STAGES])
{
	return stage_ms(ctx, kLzSizeStages, "lz_stage_ms", ms, CFLZ_STAGES);
}

// ---- the zlib stream of payloads (csrc/deflate.hip, csrc/deflate.h; the definition is tests/deflate_ref.py) --------
static const uint8_t kDeflateEmpty[11] = {0x78, 0x9C, 0x01, 0x00, 0x00, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x01};

static cfhip_deflate_result deflate_empty_result()
{
	cfhip_deflate_result r;
	memset(&r, 0, sizeof(r));
	r.bytes_out = sizeof(kDeflateEmpty);
	r.adler32 = 1u;
	return r;
}

size_t cfhip_deflate_bound(size_t n)
{
	return cfdf_bound(n);
}

// Every check of an encoder call, made before the context is touched.
static int deflate_check(cfhip_ctx* ctx, const char* what, const cfhip_lz_span* spans, size_t n, const void* out, size_t cap,
	const void* result, bool host, LzPlan* p)
{
	if (!out)
		return fail(ctx, CFHIP_E_INVALID, "%s: out is NULL", what);
	if (!result)
		return fail(ctx, CFHIP_E_INVALID, "%s: result is NULL", what);
	if (!host && ((uintptr_t)out % 4u != 0 || (uintptr_t)result % 8u != 0))
		return fail(ctx, CFHIP_E_INVALID, "%s: out must be 4-byte and result 8-byte aligned", what);
	const int rc = lz_check(ctx, what, spans, n, out, true, p);
	if (rc != CFHIP_OK)
		return rc;
	if (cap < cfdf_bound(p->total))
		return fail(ctx, CFHIP_E_CAPACITY, "%s: out holds %zu bytes, cfhip_deflate_bound(%zu) = %zu", what, cap, p->total,
			cfdf_bound(p->total));
	return CFHIP_OK;
}

// The stream of p (total > 0) into out_device (zeroed here) and the result into result_device: slices of whole groups,
// each behind the W bytes before it, the state carried on the device.
// index_device: NULL, or the stream's index entries (cfhip_deflate_indexed*), written slice by slice from the group records.
static int deflate_run(cfhip_ctx* ctx, StagingLease& lease, const LzPlan& p, hipMemcpyKind kind, uint8_t* out_device,
	unsigned long long* result_device, cfinf_entry* index_device = nullptr)
{
	const hipStream_t stream = lease.stream;
	size_t slice = 0, sort_bytes = 0;
	int rc = lz_slice_plan(ctx, p.total, CFLZ_COSTBLK, &slice, &sort_bytes);
	if (rc != CFHIP_OK)
		return rc;
	const cfdf_layout lay = cfdf_scratch(slice, sort_bytes);
	rc = reserve(ctx, &ctx->d_lz, &ctx->lz_cap, lay.total);
	if (rc != CFHIP_OK)
		return rc;
	uint8_t* base = static_cast<uint8_t*>(ctx->d_lz);
	unsigned long long* state = reinterpret_cast<unsigned long long*>(base + lay.state);
	HIP_TRY(ctx, hipMemsetAsync(out_device, 0, cfdf_bound(p.total), stream));
	for (size_t s0 = 0; s0 < p.total; s0 += slice) {
		const size_t s1 = std::min(p.total, s0 + slice);
		const size_t carry = s0 ? CFLZ_WINDOW : 0u;
		rc = lz_gather(ctx, p, s0 - carry, s1, base + lay.lz.bytes, kind, stream);
		if (rc != CFHIP_OK)
			return rc;
		hipEvent_t ev[2*CFDF_STAGES];
		rc = take_event_pairs(ctx, ev, CFDF_STAGES);
		if (rc != CFHIP_OK)
			return rc;
		const hipError_t e = cfhip_launch_deflate_slice(base, &lay, sort_bytes, (uint32_t)carry, (uint32_t)(s1 - s0), s0 == 0,
			s1 == p.total, out_device, ev, stream);
		if (e != hipSuccess)
			return fail(ctx, CFHIP_E_DEVICE, "deflate launch: %s", hipGetErrorString(e));
		if (index_device) {
			const hipError_t ie = cfhip_launch_zindex(reinterpret_cast<const uint32_t*>(base + lay.blk), (uint32_t)(s1 - s0),
				s0/CFLZ_CHUNK, index_device, stream);
			if (ie != hipSuccess)
				return fail(ctx, CFHIP_E_DEVICE, "deflate index launch: %s", hipGetErrorString(ie));
		}
	}
	const hipError_t e = cfhip_launch_deflate_final(state, (unsigned long long)p.total, out_device, result_device, stream);
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "deflate launch: %s", hipGetErrorString(e));
	return CFHIP_OK;
}

static int deflate_host(cfhip_ctx* ctx, StagingLease& lease, const LzPlan& p, void* out, cfhip_deflate_result* result,
	cfhip_zindex_entry* index = nullptr)
{
	static_assert(sizeof(cfhip_deflate_result) == 9*sizeof(unsigned long long), "the final kernel's words are the struct");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	begin_call(ctx, lease.stream, kDeflateStages);
	const size_t res_off = result_offset(cfdf_bound(p.total));
	const size_t entries = (p.total + CFLZ_CHUNK - 1u)/CFLZ_CHUNK;      // the index lies behind the result
	int rc = lease.acquire();
	if (rc == CFHIP_OK)
		rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, res_off + 256u + (index ? entries*sizeof(cfinf_entry) : 0u));
	if (rc != CFHIP_OK)
		return rc;
	uint8_t* d_out = static_cast<uint8_t*>(ctx->d_out);
	unsigned long long* d_res = reinterpret_cast<unsigned long long*>(d_out + res_off);
	cfinf_entry* d_index = index ? reinterpret_cast<cfinf_entry*>(d_out + res_off + 256u) : nullptr;
	rc = deflate_run(ctx, lease, p, hipMemcpyHostToDevice, d_out, d_res, d_index);
	if (rc != CFHIP_OK)
		return rc;
	if (index)
		HIP_TRY(ctx, hipMemcpyAsync(index, d_index, entries*sizeof(cfinf_entry), hipMemcpyDeviceToHost, lease.stream));
	return download_sized(ctx, lease, "deflate", d_res, d_out, cfdf_bound(p.total), out, result);
}

int cfhip_deflate(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out, size_t cap,
	cfhip_deflate_result* result)
{
	return guarded(ctx, "deflate", [&]() -> int {
		LzPlan p;
		const int rc = deflate_check(ctx, "deflate", spans, n_spans, out, cap, result, true, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!p.total) {
			memcpy(out, kDeflateEmpty, sizeof(kDeflateEmpty));
			*result = deflate_empty_result();
			return CFHIP_OK;
		}
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		StagingLease lease(ctx, ctx->stream);
		return deflate_host(ctx, lease, p, out, result);
	});
}

int cfhip_deflate_device(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out_device, size_t cap,
	cfhip_deflate_result* result_device, void* stream_)
{
	return guarded(ctx, "deflate_device", [&]() -> int {
		LzPlan p;
		int rc = deflate_check(ctx, "deflate_device", spans, n_spans, out_device, cap, result_device, false, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		begin_call(ctx, lease.stream, kDeflateStages);
		if (!p.total) {
			// both sources are static: the copies may outlive the call
			static const cfhip_deflate_result empty = deflate_empty_result();
			HIP_TRY(ctx, hipMemcpyAsync(out_device, kDeflateEmpty, sizeof(kDeflateEmpty), hipMemcpyHostToDevice, lease.stream));
			HIP_TRY(ctx, hipMemcpyAsync(result_device, &empty, sizeof(empty), hipMemcpyHostToDevice, lease.stream));
		} else {
			rc = lease.acquire();
			if (rc == CFHIP_OK)
				rc = deflate_run(ctx, lease, p, hipMemcpyDeviceToDevice, static_cast<uint8_t*>(out_device),
					reinterpret_cast<unsigned long long*>(result_device));
			if (rc != CFHIP_OK)
				return rc;
		}
		return lease.done(!stream_);
	});
}

int cfhip_deflate_stage_ms(cfhip_ctx* ctx, float ms[CFDF_STAGES])
{
	return stage_ms(ctx, kDeflateStages, "deflate_stage_ms", ms, CFDF_STAGES);
}

int cfhip_deflate_code_lengths(cfhip_ctx* ctx, const uint32_t* counts, uint32_t n, uint32_t limit, uint8_t* lengths)
{
	return guarded(ctx, "deflate_code_lengths", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		if (!counts || !lengths)
			return fail(ctx, CFHIP_E_INVALID, "deflate_code_lengths: counts or lengths is NULL");
		if (n < 2u || n > 288u || limit < 1u || limit > (uint32_t)CFDF_LIMIT || (1u << limit) < n)
			return fail(ctx, CFHIP_E_INVALID, "deflate_code_lengths: %u symbols at limit %u", n, limit);
		unsigned long long sum = 0;
		for (uint32_t i = 0; i < n; ++i)
			sum += counts[i];
		if (sum + 2u >= 1ull << 32)
			return fail(ctx, CFHIP_E_INVALID, "deflate_code_lengths: the counts sum to 2^32 or more");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		begin_call(ctx, lease.stream, kDeflateStages.kernel);     // the encoder's kernel name, and no stage log
		int rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_lz, &ctx->lz_cap, 4096u);
		if (rc != CFHIP_OK)
			return rc;
		uint32_t* d_counts = static_cast<uint32_t*>(ctx->d_lz);
		uint8_t* d_lengths = static_cast<uint8_t*>(ctx->d_lz) + 2048u;
		HIP_TRY(ctx, hipMemcpyAsync(d_counts, counts, 4u*n, hipMemcpyHostToDevice, lease.stream));
		rc = timed(ctx, lease.stream, "deflate_code_lengths", [&] {
			return cfhip_launch_deflate_code_lengths(d_counts, n, limit, d_lengths, lease.stream);
		});
		if (rc != CFHIP_OK)
			return rc;
		HIP_TRY(ctx, hipMemcpyAsync(lengths, d_lengths, n, hipMemcpyDeviceToHost, lease.stream));
		return lease.done(true);
	});
}

// ---- indexed zlib streams and their inflate (csrc/inflate.hip, csrc/inflate.h; the definition is tests/inflate_ref.py) --
static_assert(sizeof(cfhip_zindex_entry) == sizeof(cfinf_entry) && sizeof(cfinf_entry) == 16, "the kernels' entry is the struct");

size_t cfhip_zindex_entries(size_t n)
{
	return n/CFINF_CHUNK + (n % CFINF_CHUNK ? 1u : 0u);
}

// The checks cfhip_deflate_indexed* add to deflate_check's.
static int zindex_check(cfhip_ctx* ctx, const char* what, const LzPlan& p, const void* index, size_t index_entries, bool host)
{
	const size_t need = cfhip_zindex_entries(p.total);
	if (need && !index)
		return fail(ctx, CFHIP_E_INVALID, "%s: index is NULL", what);
	if (!host && (uintptr_t)index % 8u != 0)
		return fail(ctx, CFHIP_E_INVALID, "%s: index must be 8-byte aligned", what);
	if (index_entries < need)
		return fail(ctx, CFHIP_E_CAPACITY, "%s: index holds %zu entries, cfhip_zindex_entries(%zu) = %zu", what, index_entries,
			p.total, need);
	return CFHIP_OK;
}

int cfhip_deflate_indexed(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out, size_t cap,
	cfhip_zindex_entry* index, size_t index_entries, cfhip_deflate_result* result)
{
	return guarded(ctx, "deflate_indexed", [&]() -> int {
		LzPlan p;
		int rc = deflate_check(ctx, "deflate_indexed", spans, n_spans, out, cap, result, true, &p);
		if (rc == CFHIP_OK)
			rc = zindex_check(ctx, "deflate_indexed", p, index, index_entries, true);
		if (rc != CFHIP_OK)
			return rc;
		if (!p.total) {
			memcpy(out, kDeflateEmpty, sizeof(kDeflateEmpty));
			*result = deflate_empty_result();
			return CFHIP_OK;
		}
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		StagingLease lease(ctx, ctx->stream);
		return deflate_host(ctx, lease, p, out, result, index);
	});
}

int cfhip_deflate_indexed_device(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out_device, size_t cap,
	cfhip_zindex_entry* index_device, size_t index_entries, cfhip_deflate_result* result_device, void* stream_)
{
	return guarded(ctx, "deflate_indexed_device", [&]() -> int {
		LzPlan p;
		int rc = deflate_check(ctx, "deflate_indexed_device", spans, n_spans, out_device, cap, result_device, false, &p);
		if (rc == CFHIP_OK)
			rc = zindex_check(ctx, "deflate_indexed_device", p, index_device, index_entries, false);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		begin_call(ctx, lease.stream, kDeflateStages);
		if (!p.total) {
			static const cfhip_deflate_result empty = deflate_empty_result();
			HIP_TRY(ctx, hipMemcpyAsync(out_device, kDeflateEmpty, sizeof(kDeflateEmpty), hipMemcpyHostToDevice, lease.stream));
			HIP_TRY(ctx, hipMemcpyAsync(result_device, &empty, sizeof(empty), hipMemcpyHostToDevice, lease.stream));
		} else {
			rc = lease.acquire();
			if (rc == CFHIP_OK)
				rc = deflate_run(ctx, lease, p, hipMemcpyDeviceToDevice, static_cast<uint8_t*>(out_device),
					reinterpret_cast<unsigned long long*>(result_device), reinterpret_cast<cfinf_entry*>(index_device));
			if (rc != CFHIP_OK)
				return rc;
		}
		return lease.done(!stream_);
	});
}

static const char* const kInflateClass[8] = {"no", "wrapper", "index", "block header", "code", "distance", "overrun",
	"checksum"};

// Every check of an inflate call, made before the context is touched.
static int inflate_check(cfhip_ctx* ctx, const char* what, const void* z, size_t zbytes, const void* index,
	size_t index_entries, const void* out, size_t out_bytes, const void* result, bool host)
{
	if (!z)
		return fail(ctx, CFHIP_E_INVALID, "%s: zstream is NULL", what);
	if (!result)
		return fail(ctx, CFHIP_E_INVALID, "%s: result is NULL", what);
	if (out_bytes && !out)
		return fail(ctx, CFHIP_E_INVALID, "%s: out is NULL", what);
	if (out_bytes >= ((size_t)1 << 31) || zbytes > ((size_t)1 << 32))
		return fail(ctx, CFHIP_E_CAPACITY, "%s: 2^31 output bytes or more, or a stream above 2^32 bytes", what);
	const size_t need = cfhip_zindex_entries(out_bytes);
	if (need && !index)
		return fail(ctx, CFHIP_E_INVALID, "%s: index is NULL", what);
	if (!host && ((uintptr_t)out % 4u != 0 || (uintptr_t)result % 8u != 0 || (uintptr_t)index % 8u != 0))
		return fail(ctx, CFHIP_E_INVALID, "%s: out must be 4-byte, index and result 8-byte aligned", what);
	if (index_entries < need)
		return fail(ctx, CFHIP_E_CAPACITY, "%s: index holds %zu entries, cfhip_zindex_entries(%zu) = %zu", what, index_entries,
			out_bytes, need);
	return CFHIP_OK;
}

// The stream at z_device into out_device and the result into result_device: the output in slices of whole groups, the
// state carried on the device.
static int inflate_run(cfhip_ctx* ctx, StagingLease& lease, const uint8_t* z_device, size_t zbytes,
	const cfinf_entry* index_device, uint8_t* out_device, size_t out_bytes, unsigned long long* result_device)
{
	const hipStream_t stream = lease.stream;
	const size_t slice = std::min(lz_slice_of(ctx), (std::max(out_bytes, (size_t)1) + CFLZ_COSTBLK - 1u)/CFLZ_COSTBLK*CFLZ_COSTBLK);
	const cfinf_layout lay = cfinf_scratch(slice);
	int rc = reserve(ctx, &ctx->d_lz, &ctx->lz_cap, lay.total);
	if (rc != CFHIP_OK)
		return rc;
	uint8_t* base = static_cast<uint8_t*>(ctx->d_lz);
	size_t at = 0;
	do {
		const size_t end = std::min(out_bytes, at + slice);
		hipEvent_t ev[2*CFINF_STAGES];
		rc = take_event_pairs(ctx, ev, CFINF_STAGES);
		if (rc != CFHIP_OK)
			return rc;
		const hipError_t e = cfhip_launch_inflate_slice(base, &lay, z_device, zbytes, index_device, out_bytes, at,
			(uint32_t)(end - at), at == 0, out_device, ev, stream);
		if (e != hipSuccess)
			return fail(ctx, CFHIP_E_DEVICE, "inflate launch: %s", hipGetErrorString(e));
		at = end;
	} while (at < out_bytes);
	const hipError_t e = cfhip_launch_inflate_final(reinterpret_cast<const unsigned long long*>(base + lay.state), z_device,
		zbytes, out_bytes, result_device, stream);
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "inflate launch: %s", hipGetErrorString(e));
	return CFHIP_OK;
}

// A stream of no output bytes on the host: the walk from bit 16 through everything that produces no output, the
// trailer, Adler-32 = 1 -- the kernels' routine (inflate.h), one lane wide.
static void inflate_empty(const uint8_t* z, size_t zbytes, cfhip_inflate_result* r)
{
	std::unique_ptr<CfinfWork> w(new CfinfWork);
	memset(r, 0, sizeof(*r));
	r->bytes_in = zbytes;
	r->status = cfinf_chunk(*w, z, zbytes, nullptr, 0u, 0u, 0u, 0u, 1u);
	if (r->status == CFINF_OK) {
		const uint8_t* t = z + zbytes - 4u;
		if (((uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3]) != 1u)
			r->status = CFINF_E_CHECKSUM;
		else
			r->adler32 = 1u;
	}
}

static int inflate_verdict(cfhip_ctx* ctx, const cfhip_inflate_result& r)
{
	if (r.status == CFINF_OK)
		return CFHIP_OK;
	return fail(ctx, CFHIP_E_DATA, "inflate: %s error in chunk %u", kInflateClass[r.status & 7u], r.bad_chunk);
}

int cfhip_inflate(cfhip_ctx* ctx, const void* zstream, size_t zbytes, const cfhip_zindex_entry* index, size_t index_entries,
	void* out, size_t out_bytes, cfhip_inflate_result* result)
{
	static_assert(sizeof(cfhip_inflate_result) == 7*sizeof(unsigned long long), "the final kernel's words are the struct");
	static_assert(CFINF_OK == 0, "download_checked's status of no error");
	return guarded(ctx, "inflate", [&]() -> int {
		int rc = inflate_check(ctx, "inflate", zstream, zbytes, index, index_entries, out, out_bytes, result, true);
		if (rc != CFHIP_OK)
			return rc;
		if (!out_bytes) {
			inflate_empty(static_cast<const uint8_t*>(zstream), zbytes, result);
			return inflate_verdict(ctx, *result);
		}
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		begin_call(ctx, lease.stream, kInflateStages);
		// the stream and behind it the index; the output and behind it the result
		const size_t entries = cfhip_zindex_entries(out_bytes);
		const size_t idx_off = (zbytes + 255u)/256u*256u, res_off = result_offset(out_bytes);
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, idx_off + entries*sizeof(cfinf_entry));
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, res_off + 256u);
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d_z = static_cast<uint8_t*>(ctx->d_src);
		uint8_t* d_out = static_cast<uint8_t*>(ctx->d_out);
		unsigned long long* d_res = reinterpret_cast<unsigned long long*>(d_out + res_off);
		if (zbytes)
			HIP_TRY(ctx, hipMemcpyAsync(d_z, zstream, zbytes, hipMemcpyHostToDevice, lease.stream));
		HIP_TRY(ctx, hipMemcpyAsync(d_z + idx_off, index, entries*sizeof(cfinf_entry), hipMemcpyHostToDevice, lease.stream));
		rc = inflate_run(ctx, lease, d_z, zbytes, reinterpret_cast<const cfinf_entry*>(d_z + idx_off), d_out, out_bytes, d_res);
		if (rc != CFHIP_OK)
			return rc;
		rc = download_checked(ctx, lease, d_res, d_out, out_bytes, out, result);
		return rc == CFHIP_OK ? inflate_verdict(ctx, *result) : rc;
	});
}

int cfhip_inflate_device(cfhip_ctx* ctx, const void* zstream_device, size_t zbytes, const cfhip_zindex_entry* index_device,
	size_t index_entries, void* out_device, size_t out_bytes, cfhip_inflate_result* result_device, void* stream_)
{
	return guarded(ctx, "inflate_device", [&]() -> int {
		int rc = inflate_check(ctx, "inflate_device", zstream_device, zbytes, index_device, index_entries, out_device, out_bytes,
			result_device, false);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		begin_call(ctx, lease.stream, kInflateStages);
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = inflate_run(ctx, lease, static_cast<const uint8_t*>(zstream_device), zbytes,
				reinterpret_cast<const cfinf_entry*>(index_device), static_cast<uint8_t*>(out_device), out_bytes,
				reinterpret_cast<unsigned long long*>(result_device));
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

int cfhip_inflate_stage_ms(cfhip_ctx* ctx, float ms[CFINF_STAGES])
{
	return stage_ms(ctx, kInflateStages, "inflate_stage_ms", ms, CFINF_STAGES);
}

// ---- LZ4 frames, both ways (csrc/lz4.hip, csrc/lz4.h; the definition is tests/lz4_ref.py) ---------------------------
size_t cfhip_lz4_bound(size_t n)
{
	return cflz4_bound(n);
}

// Every check of an encoder call, made before the context is touched.
static int lz4_check(cfhip_ctx* ctx, const char* what, const cfhip_lz_span* spans, size_t n, const void* out, size_t cap,
	const void* result, bool host, LzPlan* p)
{
	if (!out)
		return fail(ctx, CFHIP_E_INVALID, "%s: out is NULL", what);
	if (!result)
		return fail(ctx, CFHIP_E_INVALID, "%s: result is NULL", what);
	if (!host && (uintptr_t)result % 8u != 0)
		return fail(ctx, CFHIP_E_INVALID, "%s: result must be 8-byte aligned", what);
	const int rc = lz_check(ctx, what, spans, n, out, true, p);
	if (rc != CFHIP_OK)
		return rc;
	if (cap < cflz4_bound(p->total))
		return fail(ctx, CFHIP_E_CAPACITY, "%s: out holds %zu bytes, cfhip_lz4_bound(%zu) = %zu", what, cap, p->total,
			cflz4_bound(p->total));
	return CFHIP_OK;
}

static cfhip_lz4_result lz4_empty_result()
{
	cfhip_lz4_result r;
	memset(&r, 0, sizeof(r));
	r.bytes_out = CFLZ4_HEADER + 4u;
	return r;
}

static void lz4_empty_frame(uint8_t out[CFLZ4_HEADER + 4u])
{
	cflz4_write_header(out, 0u);
	memset(out + CFLZ4_HEADER, 0, 4u);
}

// The frame of p (total > 0) into out_device and the result into result_device: slices of whole blocks without a carry
// (blocks are independent), the state carried on the device.
static int lz4_run(cfhip_ctx* ctx, StagingLease& lease, const LzPlan& p, hipMemcpyKind kind, uint8_t* out_device,
	unsigned long long* result_device)
{
	const hipStream_t stream = lease.stream;
	size_t slice = 0, sort_bytes = 0;
	int rc = lz_slice_plan(ctx, p.total, CFLZ4_BLOCK, &slice, &sort_bytes);
	if (rc != CFHIP_OK)
		return rc;
	const cflz4_layout lay = cflz4_scratch(slice, sort_bytes);
	rc = reserve(ctx, &ctx->d_lz, &ctx->lz_cap, lay.total);
	if (rc != CFHIP_OK)
		return rc;
	uint8_t* base = static_cast<uint8_t*>(ctx->d_lz);
	for (size_t s0 = 0; s0 < p.total; s0 += slice) {
		const size_t s1 = std::min(p.total, s0 + slice);
		rc = lz_gather(ctx, p, s0, s1, base + lay.lz.bytes, kind, stream);
		if (rc != CFHIP_OK)
			return rc;
		hipEvent_t ev[2*(CFLZ4_STAGES - 1)];
		rc = take_event_pairs(ctx, ev, CFLZ4_STAGES - 1);
		if (rc != CFHIP_OK)
			return rc;
		const hipError_t e = cfhip_launch_lz4_slice(base, &lay, sort_bytes, (uint32_t)(s1 - s0), s0 == 0, out_device, ev, stream);
		if (e != hipSuccess)
			return fail(ctx, CFHIP_E_DEVICE, "lz4_encode launch: %s", hipGetErrorString(e));
	}
	hipEvent_t ev[2];
	rc = take_event_pairs(ctx, ev, 1);
	if (rc != CFHIP_OK)
		return rc;
	const hipError_t e = cfhip_launch_lz4_final(reinterpret_cast<const unsigned long long*>(base + lay.state),
		(unsigned long long)p.total, out_device, result_device, ev, stream);
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "lz4_encode launch: %s", hipGetErrorString(e));
	return CFHIP_OK;
}

int cfhip_lz4_encode(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out, size_t cap,
	cfhip_lz4_result* result)
{
	static_assert(sizeof(cfhip_lz4_result) == 7*sizeof(unsigned long long), "the final kernel's words are the struct");
	return guarded(ctx, "lz4_encode", [&]() -> int {
		LzPlan p;
		int rc = lz4_check(ctx, "lz4_encode", spans, n_spans, out, cap, result, true, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!p.total) {
			lz4_empty_frame(static_cast<uint8_t*>(out));
			*result = lz4_empty_result();
			return CFHIP_OK;
		}
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		begin_call(ctx, lease.stream, kLz4EncodeStages);
		const size_t res_off = result_offset(cflz4_bound(p.total));
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, res_off + 256u);
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d_out = static_cast<uint8_t*>(ctx->d_out);
		unsigned long long* d_res = reinterpret_cast<unsigned long long*>(d_out + res_off);
		rc = lz4_run(ctx, lease, p, hipMemcpyHostToDevice, d_out, d_res);
		if (rc != CFHIP_OK)
			return rc;
		return download_sized(ctx, lease, "lz4_encode", d_res, d_out, cflz4_bound(p.total), out, result);
	});
}

int cfhip_lz4_encode_device(cfhip_ctx* ctx, const cfhip_lz_span* spans, size_t n_spans, void* out_device, size_t cap,
	cfhip_lz4_result* result_device, void* stream_)
{
	return guarded(ctx, "lz4_encode_device", [&]() -> int {
		LzPlan p;
		int rc = lz4_check(ctx, "lz4_encode_device", spans, n_spans, out_device, cap, result_device, false, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		begin_call(ctx, lease.stream, kLz4EncodeStages);
		if (!p.total) {
			// both sources are static: the copies may outlive the call
			static const cfhip_lz4_result empty = lz4_empty_result();
			static const struct Frame { uint8_t b[CFLZ4_HEADER + 4u]; Frame() { lz4_empty_frame(b); } } frame;
			HIP_TRY(ctx, hipMemcpyAsync(out_device, frame.b, sizeof(frame.b), hipMemcpyHostToDevice, lease.stream));
			HIP_TRY(ctx, hipMemcpyAsync(result_device, &empty, sizeof(empty), hipMemcpyHostToDevice, lease.stream));
		} else {
			rc = lease.acquire();
			if (rc == CFHIP_OK)
				rc = lz4_run(ctx, lease, p, hipMemcpyDeviceToDevice, static_cast<uint8_t*>(out_device),
					reinterpret_cast<unsigned long long*>(result_device));
			if (rc != CFHIP_OK)
				return rc;
		}
		return lease.done(!stream_);
	});
}

int cfhip_lz4_encode_stage_ms(cfhip_ctx* ctx, float* ms, size_t n)
{
	return stage_ms(ctx, kLz4EncodeStages, "cfhip_lz4_encode", ms, n);
}

static const char* const kLz4Class[8] = {"no", "header", "unsupported", "blocks", "checksum", "sequence", "offset", "size"};

// Every check of a decoder call, made before the context is touched.
static int lz4d_check(cfhip_ctx* ctx, const char* what, const void* frame, size_t bytes, const void* out, size_t out_bytes,
	const void* result, bool host)
{
	if (!frame)
		return fail(ctx, CFHIP_E_INVALID, "%s: frame is NULL", what);
	if (!result)
		return fail(ctx, CFHIP_E_INVALID, "%s: result is NULL", what);
	if (out_bytes && !out)
		return fail(ctx, CFHIP_E_INVALID, "%s: out is NULL", what);
	if (out_bytes >= ((size_t)1 << 31) || bytes > ((size_t)1 << 32))
		return fail(ctx, CFHIP_E_CAPACITY, "%s: 2^31 output bytes or more, or a frame above 2^32 bytes", what);
	if (!host && ((uintptr_t)out % 4u != 0 || (uintptr_t)result % 8u != 0))
		return fail(ctx, CFHIP_E_INVALID, "%s: out must be 4-byte and result 8-byte aligned", what);
	return CFHIP_OK;
}

static int lz4d_run(cfhip_ctx* ctx, StagingLease& lease, const uint8_t* z_device, size_t bytes, uint8_t* out_device,
	size_t out_bytes, unsigned long long* result_device)
{
	const cflz4_dlayout lay = cflz4_dscratch((out_bytes + CFLZ4_BLOCK - 1u)/CFLZ4_BLOCK);
	int rc = reserve(ctx, &ctx->d_lz, &ctx->lz_cap, lay.total);
	if (rc != CFHIP_OK)
		return rc;
	hipEvent_t ev[2*CFLZ4_DSTAGES];
	rc = take_event_pairs(ctx, ev, CFLZ4_DSTAGES);
	if (rc != CFHIP_OK)
		return rc;
	const hipError_t e = cfhip_launch_lz4_decode(static_cast<uint8_t*>(ctx->d_lz), &lay, z_device, bytes, out_device, out_bytes,
		result_device, ev, lease.stream);
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "lz4_decode launch: %s", hipGetErrorString(e));
	return CFHIP_OK;
}

// A frame of no output bytes on the host: the header and the frame's end -- the kernels' routines (lz4.h).
static void lz4d_empty(const uint8_t* z, size_t bytes, cfhip_lz4_decode_result* r)
{
	memset(r, 0, sizeof(*r));
	r->bytes_in = bytes;
	cflz4_header h;
	r->status = cflz4_parse_header(z, bytes, 0u, &h);
	if (r->status == CFLZ4_OK) {
		r->content_checksum = h.content_checksum;
		r->status = cflz4_frame_end(z, bytes, h.content_checksum, h.length);
	}
}

static int lz4d_verdict(cfhip_ctx* ctx, const cfhip_lz4_decode_result& r)
{
	if (r.status == CFLZ4_OK)
		return CFHIP_OK;
	return fail(ctx, CFHIP_E_DATA, "lz4_decode: %s error in block %u", kLz4Class[r.status & 7u], r.bad_block);
}

int cfhip_lz4_decode(cfhip_ctx* ctx, const void* frame, size_t bytes, void* out, size_t out_bytes,
	cfhip_lz4_decode_result* result)
{
	static_assert(sizeof(cfhip_lz4_decode_result) == 9*sizeof(unsigned long long), "the final kernel's words are the struct");
	static_assert(CFLZ4_OK == 0, "download_checked's status of no error");
	return guarded(ctx, "lz4_decode", [&]() -> int {
		int rc = lz4d_check(ctx, "lz4_decode", frame, bytes, out, out_bytes, result, true);
		if (rc != CFHIP_OK)
			return rc;
		if (!out_bytes) {
			lz4d_empty(static_cast<const uint8_t*>(frame), bytes, result);
			return lz4d_verdict(ctx, *result);
		}
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		begin_call(ctx, lease.stream, kLz4DecodeStages);
		const size_t res_off = result_offset(out_bytes);
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, std::max(bytes, (size_t)1));
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, res_off + 256u);
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d_z = static_cast<uint8_t*>(ctx->d_src);
		uint8_t* d_out = static_cast<uint8_t*>(ctx->d_out);
		unsigned long long* d_res = reinterpret_cast<unsigned long long*>(d_out + res_off);
		if (bytes)
			HIP_TRY(ctx, hipMemcpyAsync(d_z, frame, bytes, hipMemcpyHostToDevice, lease.stream));
		rc = lz4d_run(ctx, lease, d_z, bytes, d_out, out_bytes, d_res);
		if (rc != CFHIP_OK)
			return rc;
		rc = download_checked(ctx, lease, d_res, d_out, out_bytes, out, result);
		return rc == CFHIP_OK ? lz4d_verdict(ctx, *result) : rc;
	});
}

int cfhip_lz4_decode_device(cfhip_ctx* ctx, const void* frame_device, size_t bytes, void* out_device, size_t out_bytes,
	cfhip_lz4_decode_result* result_device, void* stream_)
{
	return guarded(ctx, "lz4_decode_device", [&]() -> int {
		int rc = lz4d_check(ctx, "lz4_decode_device", frame_device, bytes, out_device, out_bytes, result_device, false);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		begin_call(ctx, lease.stream, kLz4DecodeStages);
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = lz4d_run(ctx, lease, static_cast<const uint8_t*>(frame_device), bytes, static_cast<uint8_t*>(out_device),
				out_bytes, reinterpret_cast<unsigned long long*>(result_device));
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

int cfhip_lz4_decode_stage_ms(cfhip_ctx* ctx, float* ms, size_t n)
{
	return stage_ms(ctx, kLz4DecodeStages, "cfhip_lz4_decode", ms, n);
}

// ---- PNG files of images (csrc/png.hip, csrc/png.h; the definition is tests/png_ref.py) ----------------------------
size_t cfhip_png_bound(uint32_t width, uint32_t height, int color_type, int bit_depth, int color_space)
{
	if (color_space != CFHIP_COLOR_LINEAR && color_space != CFHIP_COLOR_SRGB)
		return 0;
	const uint64_t b = cfpng_bound(width, height, color_type, bit_depth, color_space == CFHIP_COLOR_SRGB);
	return b > (uint64_t)SIZE_MAX ? SIZE_MAX : (size_t)b;
}

struct PngPlan {
	uint32_t bpp = 0;
	size_t texel = 0, filtered = 0, bound = 0;
	int srgb = 0;
};

// Every check of a call, made before the context is touched.
static int png_check(cfhip_ctx* ctx, const char* what, const void* pixels, int pixel_type, size_t pitch, uint32_t width,
	uint32_t height, int color_type, int bit_depth, int color_space, const void* out, size_t cap, const void* result, bool host,
	PngPlan* p)
{
	if (!out)
		return fail(ctx, CFHIP_E_INVALID, "%s: out is NULL", what);
	if (!result)
		return fail(ctx, CFHIP_E_INVALID, "%s: result is NULL", what);
	if (!pixels)
		return fail(ctx, CFHIP_E_INVALID, "%s: pixels is NULL", what);
	if (!width || !height)
		return fail(ctx, CFHIP_E_INVALID, "%s: empty image %ux%u", what, width, height);
	p->texel = pixel_bytes(pixel_type);
	if (!p->texel)
		return fail(ctx, CFHIP_E_INVALID, "%s: pixel type %d", what, pixel_type);
	if (color_space != CFHIP_COLOR_LINEAR && color_space != CFHIP_COLOR_SRGB)
		return fail(ctx, CFHIP_E_INVALID, "%s: colour space %d", what, color_space);
	if (color_type == CFPNG_PALETTE)
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: palette images are not written", what);
	if (!cfpng_channels(color_type))
		return fail(ctx, CFHIP_E_INVALID, "%s: colour type %d", what, color_type);
	if (bit_depth == 1 || bit_depth == 2 || bit_depth == 4)
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: bit depth %d is not written (8 or 16)", what, bit_depth);
	if (bit_depth != 8 && bit_depth != 16)
		return fail(ctx, CFHIP_E_INVALID, "%s: bit depth %d", what, bit_depth);
	if (pitch < (size_t)width*p->texel)
		return fail(ctx, CFHIP_E_INVALID, "%s: pitch %zu < %zu", what, pitch, (size_t)width*p->texel);
	if (!host && ((uintptr_t)pixels % p->texel || pitch % p->texel))
		return fail(ctx, CFHIP_E_INVALID, "%s: pixels or the pitch not aligned to the texel size", what);
	if (!host && (uintptr_t)result % 8u != 0)
		return fail(ctx, CFHIP_E_INVALID, "%s: result must be 8-byte aligned", what);
	p->bpp = cfpng_bpp(color_type, bit_depth);
	p->srgb = color_space == CFHIP_COLOR_SRGB;
	const uint64_t n = cfpng_filtered_bytes(width, height, p->bpp);
	if (n >= ((uint64_t)1 << 31))
		return fail(ctx, CFHIP_E_CAPACITY, "%s: 2^31 filtered bytes or more", what);
	p->filtered = (size_t)n;
	p->bound = (size_t)cfpng_bound(width, height, color_type, bit_depth, p->srgb);
	if (cap < p->bound)
		return fail(ctx, CFHIP_E_CAPACITY, "%s: out holds %zu bytes, cfhip_png_bound = %zu", what, cap, p->bound);
	return CFHIP_OK;
}

// The file of the image at pixels_device into out_device and the result into result_device, enqueued on the lease's stream.
static int png_run(cfhip_ctx* ctx, StagingLease& lease, const PngPlan& p, const void* pixels_device, int pixel_type, size_t pitch,
	uint32_t width, uint32_t height, int color_type, int bit_depth, uint8_t* out_device, unsigned long long* result_device)
{
	static_assert(sizeof(cfhip_png_result) == 15*sizeof(unsigned long long), "the final kernel's words are the struct");
	static_assert(offsetof(cfhip_png_result, deflate) == 48, "the final kernel's words are the struct");
	const hipStream_t stream = lease.stream;
	cfpng_head head;
	cfpng_write_head(&head, width, height, color_type, bit_depth, p.srgb);
	const size_t zbound = cfdf_bound(p.filtered);
	if (head.bytes + zbound + CFPNG_TAIL != p.bound)
		return fail(ctx, CFHIP_E_DEVICE, "png_encode: the bound's parts do not add up");
	// the encoder writes whole words: in place where the IDAT data starts on one, into scratch otherwise
	const bool in_place = ((uintptr_t)out_device + head.bytes) % 4u == 0;
	const cfpng_layout lay = cfpng_scratch(p.filtered, in_place ? 0u : zbound);
	int rc = reserve(ctx, &ctx->d_png, &ctx->png_cap, lay.total);
	if (rc != CFHIP_OK)
		return rc;
	uint8_t* base = static_cast<uint8_t*>(ctx->d_png);
	uint32_t* state = reinterpret_cast<uint32_t*>(base + lay.state);
	uint8_t* data = out_device + head.bytes;
	uint8_t* z = in_place ? data : base + lay.zstream;
	HIP_TRY(ctx, hipMemsetAsync(state, 0, CFPNG_S_WORDS*4u, stream));
	hipEvent_t ev[2];
	rc = take_event_pairs(ctx, ev, 1);
	if (rc != CFHIP_OK)
		return rc;
	HIP_TRY(ctx, hipEventRecord(ev[0], stream));
	hipError_t e = cfhip_launch_png_filter(pixels_device, pixel_type, pitch, width, height, color_type, bit_depth,
		base + lay.filtered, state, stream);
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "png_encode launch: %s", hipGetErrorString(e));
	HIP_TRY(ctx, hipEventRecord(ev[1], stream));
	LzPlan lz;
	cfhip_lz_span span;
	span.bytes = base + lay.filtered;
	span.n = p.filtered;
	lz.spans.push_back(span);
	lz.total = p.filtered;
	rc = deflate_run(ctx, lease, lz, hipMemcpyDeviceToDevice, z, reinterpret_cast<unsigned long long*>(state + CFPNG_S_DEFLATE));
	if (rc != CFHIP_OK)
		return rc;
	rc = take_event_pairs(ctx, ev, 1);
	if (rc != CFHIP_OK)
		return rc;
	HIP_TRY(ctx, hipEventRecord(ev[0], stream));
	e = cfhip_launch_png_crc(z, data, zbound, state, stream);
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "png_encode launch: %s", hipGetErrorString(e));
	HIP_TRY(ctx, hipEventRecord(ev[1], stream));
	rc = take_event_pairs(ctx, ev, 1);
	if (rc != CFHIP_OK)
		return rc;
	HIP_TRY(ctx, hipEventRecord(ev[0], stream));
	e = cfhip_launch_png_final(&head, z, p.filtered, state, out_device, result_device, stream);
	if (e != hipSuccess)
		return fail(ctx, CFHIP_E_DEVICE, "png_encode launch: %s", hipGetErrorString(e));
	HIP_TRY(ctx, hipEventRecord(ev[1], stream));
	return CFHIP_OK;
}

int cfhip_png_encode(cfhip_ctx* ctx, const void* pixels, int pixel_type, size_t pitch_bytes, uint32_t width, uint32_t height,
	int color_type, int bit_depth, int color_space, void* out, size_t cap, cfhip_png_result* result)
{
	return guarded(ctx, "png_encode", [&]() -> int {
		PngPlan p;
		int rc = png_check(ctx, "png_encode", pixels, pixel_type, pitch_bytes, width, height, color_type, bit_depth, color_space,
			out, cap, result, true, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		begin_call(ctx, lease.stream, kPngStages);
		// the file starts where its IDAT data falls on a word; the result lies behind it, 256-byte aligned
		const size_t lead = (4u - cfpng_data_offset(p.srgb) % 4u) % 4u;
		const size_t res_off = result_offset(lead + p.bound);
		const size_t row = (size_t)width*p.texel;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, row*height);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, res_off + 256u);
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d_file = static_cast<uint8_t*>(ctx->d_out) + lead;
		unsigned long long* d_res = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(ctx->d_out) + res_off);
		HIP_TRY(ctx, hipMemcpy2DAsync(ctx->d_src, row, pixels, pitch_bytes, row, height, hipMemcpyHostToDevice, lease.stream));
		rc = png_run(ctx, lease, p, ctx->d_src, pixel_type, row, width, height, color_type, bit_depth, d_file, d_res);
		if (rc != CFHIP_OK)
			return rc;
		return download_sized(ctx, lease, "png_encode", d_res, d_file, p.bound, out, result);
	});
}

int cfhip_png_encode_device(cfhip_ctx* ctx, const void* pixels_device, int pixel_type, size_t pitch_bytes, uint32_t width,
	uint32_t height, int color_type, int bit_depth, int color_space, void* out_device, size_t cap,
	cfhip_png_result* result_device, void* stream_)
{
	return guarded(ctx, "png_encode_device", [&]() -> int {
		PngPlan p;
		int rc = png_check(ctx, "png_encode_device", pixels_device, pixel_type, pitch_bytes, width, height, color_type, bit_depth,
			color_space, out_device, cap, result_device, false, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		begin_call(ctx, lease.stream, kPngStages);
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = png_run(ctx, lease, p, pixels_device, pixel_type, pitch_bytes, width, height, color_type, bit_depth,
				static_cast<uint8_t*>(out_device), reinterpret_cast<unsigned long long*>(result_device));
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

int cfhip_png_stage_ms(cfhip_ctx* ctx, float ms[CFPNG_STAGES])
{
	static_assert(CFPNG_STAGES == 1 + CFDF_STAGES + 2, "filter, the encoder's stages, crc, final");
	return stage_ms(ctx, kPngStages, "png_stage_ms", ms, CFPNG_STAGES);
}

// cfhip_rdo_target and cfhip_rdo_target_device
static int rdo_target(cfhip_ctx* ctx, const char* what, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_ex_params* ex, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats, bool host, float target_ratio,
	cfhip_rdo_target_result* result, void* stream_)
{
	return guarded(ctx, what, [&]() -> int {
		RdoPlan p;
		int rc = rdo_check(ctx, what, format, type, surfaces, n, nullptr, ex, mask_rgba, stats, host, &p);
		if (rc != CFHIP_OK)
			return rc;
		if (!n) {
			if (result)
				memset(result, 0, sizeof(*result));
			return CFHIP_OK;
		}
		if (!(target_ratio > 0.0f && target_ratio < 1.0f))
			return fail(ctx, CFHIP_E_INVALID, "%s: target_ratio %g is outside (0, 1)", what, (double)target_ratio);
		if (!result)
			return fail(ctx, CFHIP_E_INVALID, "%s: result is NULL", what);
		size_t total = 0;
		for (size_t i = 0; i < n; ++i)
			total += p.payload[i];
		if (total >= ((size_t)1 << 31))
			return fail(ctx, CFHIP_E_CAPACITY, "%s: the payloads hold 2^31 bytes or more", what);
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, host ? nullptr : stream_));
		const hipStream_t stream = lease.stream;
		// every launch of the search is timed: the call's event pairs start here and every trial adds its own; the
		// search's estimates (lz_run) belong to no stage log; the trials name the kernel
		begin_call(ctx, stream, nullptr);
		rc = lease.acquire();
		if (rc != CFHIP_OK)
			return rc;
		// the pristine payloads: scratch for the host form and for surfaces optimised in place, else the caller's
		std::vector<size_t> off(n), pix_off(n);
		size_t keep = 0, po = 0;
		for (size_t i = 0; i < n; ++i) {
			off[i] = keep;
			keep = (keep + p.payload[i] + 255u) & ~(size_t)255u;
			pix_off[i] = po;
			po = align16(po + (size_t)surfaces[i].width*p.texel[i]*surfaces[i].height);
		}
		// (the device form needs the copy only for surfaces optimised in place)
		bool keeps = host;
		for (size_t i = 0; i < n && !keeps; ++i)
			keeps = surfaces[i].out == surfaces[i].blocks;
		if (keeps)
			rc = reserve(ctx, &ctx->d_rdo_keep, &ctx->rdo_keep_cap, keep);
		cfhip_rdo_stats* d_stats = stats;
		if (host) {
			if (rc == CFHIP_OK)
				rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, keep);
			if (rc == CFHIP_OK)
				rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, po + n*sizeof(cfhip_rdo_stats));
		}
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d_keep = static_cast<uint8_t*>(ctx->d_rdo_keep);
		LzPlan plain, work;
		for (size_t i = 0; i < n; ++i) {
			const cfhip_rdo_surface& s = surfaces[i];
			cfrdo_entry& e = p.entries[i];
			if (host) {
				uint8_t* d = static_cast<uint8_t*>(ctx->d_out);
				const size_t rowb = (size_t)s.width*p.texel[i];
				HIP_TRY(ctx, hipMemcpyAsync(d_keep + off[i], s.blocks, p.payload[i], hipMemcpyHostToDevice, stream));
				if (s.row_pitch_bytes == rowb)
					HIP_TRY(ctx, hipMemcpyAsync(d + pix_off[i], s.pixels, rowb*s.height, hipMemcpyHostToDevice, stream));
				else
					HIP_TRY(ctx, hipMemcpy2DAsync(d + pix_off[i], rowb, s.pixels, s.row_pitch_bytes, rowb, s.height,
						hipMemcpyHostToDevice, stream));
				e.blocks = d_keep + off[i];
				e.out = static_cast<uint8_t*>(ctx->d_src) + off[i];
				e.pixels = d + pix_off[i];
				e.pitch = rowb;
				d_stats = reinterpret_cast<cfhip_rdo_stats*>(d + po);
			} else if (s.out == s.blocks) {
				HIP_TRY(ctx, hipMemcpyAsync(d_keep + off[i], s.blocks, p.payload[i], hipMemcpyDeviceToDevice, stream));
				e.blocks = d_keep + off[i];
			}
			plain.spans.push_back(cfhip_lz_span{e.blocks, p.payload[i]});
			work.spans.push_back(cfhip_lz_span{e.out, p.payload[i]});
		}
		plain.total = work.total = total;
		// one estimate, read back: every trial decides on the host what the next one is
		auto estimate = [&](const LzPlan& of, uint64_t* est) -> int {
			unsigned long long* d_res = nullptr;
			int r = lz_run(ctx, lease, of, hipMemcpyDeviceToDevice, nullptr, &d_res);
			if (r != CFHIP_OK)
				return r;
			cfhip_lz_stats st;
			HIP_TRY(ctx, hipMemcpyAsync(&st, d_res, sizeof(st), hipMemcpyDeviceToHost, stream));
			HIP_TRY(ctx, hipStreamSynchronize(stream));
			*est = st.est_bytes;
			return CFHIP_OK;
		};
		uint32_t current = 0xFFFFFFFFu;               // the lambda16 whose pass lies in the outputs
		auto pass = [&](uint32_t lam16) -> int {
			p.lam16 = lam16;
			current = lam16;
			return rdo_launch(ctx, lease, p, d_stats, true);
		};
		cfhip_rdo_target_result res;
		memset(&res, 0, sizeof(res));
		rc = estimate(plain, &res.est_bytes_plain);
		if (rc != CFHIP_OK)
			return rc;
		const uint64_t target = (uint64_t)std::floor((double)target_ratio*(double)res.est_bytes_plain);
		uint32_t hi = p.lam16, lo = 0u;
		uint64_t est = 0;
		rc = pass(hi);
		if (rc == CFHIP_OK)
			rc = estimate(work, &est);
		if (rc != CFHIP_OK)
			return rc;
		res.trials = 1u;
		res.est_bytes_final = est;
		res.reached = est <= target ? 1u : 0u;
		while (res.reached && hi - lo > 1u) {
			const uint32_t mid = lo + (hi - lo)/2u;
			rc = pass(mid);
			if (rc == CFHIP_OK)
				rc = estimate(work, &est);
			if (rc != CFHIP_OK)
				return rc;
			++res.trials;
			if (est <= target) {
				hi = mid;
				res.est_bytes_final = est;
			} else
				lo = mid;
		}
		if (current != hi) {
			rc = pass(hi);
			if (rc != CFHIP_OK)
				return rc;
		}
		res.lambda16 = hi;
		ctx->last_kernel = rdo_kernel(p);
		std::vector<cfhip_rdo_stats> host_stats(host ? n : 0);
		if (host) {
			HIP_TRY(ctx, hipMemcpyAsync(host_stats.data(), d_stats, n*sizeof(cfhip_rdo_stats), hipMemcpyDeviceToHost, stream));
			for (size_t i = 0; i < n; ++i)
				HIP_TRY(ctx, hipMemcpyAsync(surfaces[i].out, p.entries[i].out, p.payload[i], hipMemcpyDeviceToHost, stream));
		}
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		for (size_t i = 0; i < host_stats.size(); ++i)
			stats[i] = host_stats[i];
		*result = res;
		return CFHIP_OK;
	});
}

int cfhip_rdo_target(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_ex_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats, float target_ratio,
	cfhip_rdo_target_result* result)
{
	return rdo_target(ctx, "rdo_target", format, type, surfaces, n, params, mask_rgba, stats, true, target_ratio, result,
		nullptr);
}

int cfhip_rdo_target_device(cfhip_ctx* ctx, int format, int type, const cfhip_rdo_surface* surfaces, size_t n,
	const cfhip_rdo_ex_params* params, const uint8_t mask_rgba[4], cfhip_rdo_stats* stats_device, float target_ratio,
	cfhip_rdo_target_result* result, void* stream_)
{
	return rdo_target(ctx, "rdo_target_device", format, type, surfaces, n, params, mask_rgba, stats_device, false,
		target_ratio, result, stream_);
}

} // extern "C"

// ---- PVRTC1 4 bpp (csrc/pvrtc.hip): an entry family of its own, outside the cfhip_surface block contract ----
static bool pow2(uint32_t v) { return v && !(v & (v - 1u)); }

static int pvrtc_check(int format, int type, uint32_t width, uint32_t height, size_t* bytes)
{
	if ((format != CFHIP_FORMAT_PVRTC1_RGB_4BPP && format != CFHIP_FORMAT_PVRTC1_RGBA_4BPP) || type != CFHIP_TYPE_UNORM)
		return CFHIP_E_UNSUPPORTED;
	if (!pow2(width) || !pow2(height) || width > 32768u || height > 32768u)
		return CFHIP_E_INVALID;
	const size_t bx = width/4u > 2u ? width/4u : 2u, by = height/4u > 2u ? height/4u : 2u;
	if (bytes) *bytes = bx*by*8u;
	return CFHIP_OK;
}

// refine sweeps per quality level: each level runs the sweeps of the level below first (tests/pvrtc_ref.py
// LEVEL_SWEEPS; flag 1 = mode trial, 2 = +-1 candidates, 4 = opacity trials)
static const uint32_t kPvrtcSweeps[5][8] = {{0}, {0}, {0, 1}, {0, 1, 3, 3}, {0, 1, 3, 3, 7, 7, 7, 7}};
static const uint32_t kPvrtcNumSweeps[5] = {0, 1, 2, 4, 8};

static int pvrtc_encode_body(cfhip_ctx* ctx, StagingLease& lease, const cfhip_surface* surfaces, size_t n,
	const cfhip_params* p, bool device_mem)
{
	const char* what = device_mem ? "pvrtc_encode_device" : "pvrtc_encode";
	if (!surfaces || !n || !p)
		return fail(ctx, CFHIP_E_INVALID, "%s: no surfaces or params", what);
	int rc = pvrtc_check(p->format, p->type, 4, 4, nullptr);
	if (rc != CFHIP_OK)
		return fail(ctx, rc, "%s: (format %d, type %d) is not PVRTC1 4 bpp UNorm", what, p->format, p->type);
	if (p->quality < CFHIP_QUALITY_LOWEST || p->quality > CFHIP_QUALITY_HIGHEST)
		return fail(ctx, CFHIP_E_INVALID, "%s: bad quality %d", what, p->quality);
	if (n > (1u << 20))
		return fail(ctx, CFHIP_E_INVALID, "%s: too many surfaces", what);
	const bool rgb = p->format == CFHIP_FORMAT_PVRTC1_RGB_4BPP;
	uint32_t wmask = 0;
	for (int c = 0; c < 4; ++c)
		wmask |= p->mask_rgba[c] ? 1u << c : 0u;
	if (rgb)
		wmask &= 7u;
	std::vector<cf_pvrtc_surf> tab(n);
	std::vector<size_t> src_off(n), span(n), out_off(n), out_bytes(n);
	uint64_t blocks = 0, phase = 0;
	size_t src_total = 0, out_total = 0;
	for (size_t i = 0; i < n; ++i) {
		const cfhip_surface& s = surfaces[i];
		const size_t pb = pixel_bytes(s.pixel_type);
		size_t bytes = 0;
		if (!s.pixels || !s.out || !pb)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: bad pixels/out/pixel_type", what, i);
		if (pvrtc_check(p->format, p->type, s.width, s.height, &bytes) != CFHIP_OK)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: %ux%u is not a power-of-two size", what, i, s.width,
				s.height);
		const size_t row = (size_t)s.width*pb;
		const size_t apitch = (size_t)(s.row_pitch_bytes < 0 ? -s.row_pitch_bytes : s.row_pitch_bytes);
		if (apitch < row || apitch % pb)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: |row pitch| %zu must be >= %zu and a multiple of %zu",
				what, i, apitch, row, pb);
		if (device_mem && ((uintptr_t)s.pixels % pb))
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %zu: pixels not aligned to the pixel size", what, i);
		if (s.out_capacity < bytes)
			return fail(ctx, CFHIP_E_CAPACITY, "%s: surface %zu: out_capacity %zu < %zu", what, i, s.out_capacity,
				bytes);
		cf_pvrtc_surf& t = tab[i];
		t.pitch = (long long)s.row_pitch_bytes;
		t.pix = (uint32_t)s.pixel_type;
		t.w = s.width; t.h = s.height;
		t.bx = s.width/4u > 2u ? s.width/4u : 2u;
		t.by = s.height/4u > 2u ? s.height/4u : 2u;
		t.blk_off = (uint32_t)blocks;
		t.ph_off = (uint32_t)phase;
		t.pad = 0;
		blocks += (uint64_t)t.bx*t.by;
		phase += (uint64_t)(t.bx/2u)*(t.by/2u);
		if (blocks*16u >= (1ull << 31))
			return fail(ctx, CFHIP_E_INVALID, "%s: more than 2^31 texels in one call", what);
		span[i] = (size_t)(s.height - 1u)*apitch + row;
		src_off[i] = src_total;
		src_total += (span[i] + 255u) & ~(size_t)255u;
		out_bytes[i] = bytes;
		out_off[i] = out_total;
		out_total += (bytes + 255u) & ~(size_t)255u;
	}
	// scratch: the table, then the texels, the colour words and the modulation bytes
	const size_t tab_bytes = (n*sizeof(cf_pvrtc_surf) + 255u) & ~(size_t)255u;
	const size_t tex_off = tab_bytes, word_off = tex_off + (size_t)blocks*64u, mod_off = word_off + (size_t)blocks*4u;
	const size_t scratch = mod_off + (size_t)blocks*16u;
	const hipStream_t stream = lease.stream;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	rc = lease.acquire();
	if (rc == CFHIP_OK)
		rc = reserve(ctx, &ctx->d_pvrtc, &ctx->pvrtc_cap, scratch);
	if (rc == CFHIP_OK && !device_mem)
		rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, src_total);
	if (rc == CFHIP_OK && !device_mem)
		rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, out_total);
	if (rc != CFHIP_OK)
		return rc;
	for (size_t i = 0; i < n; ++i) {
		const cfhip_surface& s = surfaces[i];
		const size_t lead = s.row_pitch_bytes < 0 ? (size_t)(s.height - 1u)*(size_t)(-s.row_pitch_bytes) : 0u;
		if (device_mem) {
			tab[i].src = static_cast<const uint8_t*>(s.pixels);
			tab[i].out = static_cast<uint8_t*>(s.out);
		} else {
			// the whole span of rows as it lies in memory (bottom-up sources included), one copy
			uint8_t* d = static_cast<uint8_t*>(ctx->d_src) + src_off[i];
			HIP_TRY(ctx, hipMemcpyAsync(d, static_cast<const uint8_t*>(s.pixels) - lead, span[i], hipMemcpyHostToDevice,
				stream));
			tab[i].src = d + lead;
			tab[i].out = static_cast<uint8_t*>(ctx->d_out) + out_off[i];
		}
	}
	uint8_t* base = static_cast<uint8_t*>(ctx->d_pvrtc);
	const cf_pvrtc_surf* d_tab = reinterpret_cast<const cf_pvrtc_surf*>(base);
	uint32_t* tex = reinterpret_cast<uint32_t*>(base + tex_off);
	uint32_t* words = reinterpret_cast<uint32_t*>(base + word_off);
	uint8_t* mods = base + mod_off;
	// pageable source: the runtime stages the copy before returning, so `tab` may die
	HIP_TRY(ctx, hipMemcpyAsync(base, tab.data(), n*sizeof(cf_pvrtc_surf), hipMemcpyHostToDevice, stream));
	begin_call(ctx, stream, "cfhip_pvrtc_refine_kernel");
	const uint32_t nb = (uint32_t)blocks, np = (uint32_t)phase, ns = (uint32_t)n;
	// every pass of the encoder is a timed span of its own
	auto pass = [&](int k, uint32_t items, uint32_t ox, uint32_t oy, uint32_t flags) {
		return timed(ctx, stream, "pvrtc", [&] {
			return cfhip_pvrtc_launch(k, d_tab, ns, items, tex, words, mods, wmask, rgb ? 1 : 0, ox, oy, flags, stream);
		});
	};
	rc = pass(0, nb, 0, 0, 0);
	if (rc == CFHIP_OK) rc = pass(1, nb, 0, 0, 0);
	if (rc == CFHIP_OK) rc = pass(2, nb, 0, 0, 0);
	for (uint32_t sw = 0; rc == CFHIP_OK && sw < kPvrtcNumSweeps[p->quality]; ++sw)
		for (uint32_t ph = 0; rc == CFHIP_OK && ph < 4; ++ph)
			rc = pass(3, np, ph & 1u, ph >> 1, kPvrtcSweeps[p->quality][sw]);
	if (rc == CFHIP_OK) rc = pass(4, nb, 0, 0, 0);
	if (rc != CFHIP_OK)
		return rc;
	if (device_mem)
		return CFHIP_OK;
	for (size_t i = 0; i < n; ++i)
		HIP_TRY(ctx, hipMemcpyAsync(surfaces[i].out, static_cast<uint8_t*>(ctx->d_out) + out_off[i], out_bytes[i],
			hipMemcpyDeviceToHost, stream));
	return CFHIP_OK;
}

static int pvrtc_encode_impl(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n, const cfhip_params* p,
	bool device_mem, hipStream_t user_stream)
{
	return guarded(ctx, "pvrtc_encode", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		StagingLease lease(ctx, user_stream ? user_stream : ctx->stream);
		const int rc = pvrtc_encode_body(ctx, lease, surfaces, n, p, device_mem);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!user_stream);
	});
}

// the checks every PVRTC decode entry point makes before anything is enqueued
static int pvrtc_decode_check(cfhip_ctx* ctx, const char* what, int format, int type, const void* blocks,
	uint32_t width, uint32_t height, size_t* payload)
{
	const int rc = pvrtc_check(format, type, width, height, payload);
	if (rc == CFHIP_E_UNSUPPORTED)
		return fail(ctx, rc, "%s: (format %d, type %d) is not PVRTC1 4 bpp UNorm", what, format, type);
	if (rc != CFHIP_OK)
		return fail(ctx, rc, "%s: %ux%u is not a power-of-two size", what, width, height);
	if ((uint64_t)width*height > (1ull << 30))
		return fail(ctx, CFHIP_E_INVALID, "%s: surface %ux%u too large for one launch", what, width, height);
	if (!blocks)
		return fail(ctx, CFHIP_E_INVALID, "%s: blocks is NULL", what);
	return CFHIP_OK;
}

static int pvrtc_decode_launch(cfhip_ctx* ctx, int format, const void* blocks, uint32_t width, uint32_t height,
	void* out, size_t out_pitch, const void* ref, size_t ref_pitch, unsigned long long* sums, bool sse,
	hipStream_t stream)
{
	begin_call(ctx, stream, sse ? "cfhip_pvrtc_decode_sse_kernel" : "cfhip_pvrtc_decode_kernel");
	const int rgb = format == CFHIP_FORMAT_PVRTC1_RGB_4BPP ? 1 : 0;
	return timed(ctx, stream, "pvrtc", [&] {
		return cfhip_pvrtc_launch_decode(blocks, width, height, rgb, out, out_pitch, ref, ref_pitch, sums, sse ? 1 : 0,
			stream);
	});
}

extern "C" {

int cfhip_pvrtc_query(int format, int type, uint32_t width, uint32_t height, size_t* bytes)
{
	return pvrtc_check(format, type, width, height, bytes);
}

int cfhip_pvrtc_encode(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n_surfaces, const cfhip_params* params)
{
	return pvrtc_encode_impl(ctx, surfaces, n_surfaces, params, false, nullptr);
}

int cfhip_pvrtc_encode_device(cfhip_ctx* ctx, const cfhip_surface* surfaces, size_t n_surfaces,
	const cfhip_params* params, void* stream)
{
	return pvrtc_encode_impl(ctx, surfaces, n_surfaces, params, true, static_cast<hipStream_t>(stream));
}

int cfhip_pvrtc_decode(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes, uint32_t width,
	uint32_t height, void* out, size_t out_capacity)
{
	return guarded(ctx, "pvrtc_decode", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		size_t payload = 0;
		int rc = pvrtc_decode_check(ctx, "pvrtc_decode", format, type, blocks, width, height, &payload);
		if (rc != CFHIP_OK)
			return rc;
		if (!out)
			return fail(ctx, CFHIP_E_INVALID, "pvrtc_decode: out is NULL");
		if (blocks_bytes < payload)
			return fail(ctx, CFHIP_E_INVALID, "pvrtc_decode: blocks_bytes %zu < %zu", blocks_bytes, payload);
		const size_t out_bytes = (size_t)width*height*4u;
		if (out_capacity < out_bytes)
			return fail(ctx, CFHIP_E_CAPACITY, "pvrtc_decode: out_capacity %zu < %zu", out_capacity, out_bytes);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, payload);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, out_bytes);
		if (rc != CFHIP_OK)
			return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_src, blocks, payload, hipMemcpyHostToDevice, stream));
		rc = pvrtc_decode_launch(ctx, format, ctx->d_src, width, height, ctx->d_out, (size_t)width*4u, nullptr, 0, nullptr,
			false, stream);
		if (rc != CFHIP_OK)
			return rc;
		HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_out, out_bytes, hipMemcpyDeviceToHost, stream));
		return lease.done(true);
	});
}

int cfhip_pvrtc_decode_device(cfhip_ctx* ctx, int format, int type, const void* blocks, uint32_t width,
	uint32_t height, void* out, size_t out_pitch_bytes, void* stream_)
{
	return guarded(ctx, "pvrtc_decode_device", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		int rc = pvrtc_decode_check(ctx, "pvrtc_decode_device", format, type, blocks, width, height, nullptr);
		if (rc != CFHIP_OK)
			return rc;
		if (!out || out_pitch_bytes < (size_t)width*4u || ((uintptr_t)out & 3u) || (out_pitch_bytes & 3u) ||
			((uintptr_t)blocks & 3u))
			return fail(ctx, CFHIP_E_INVALID, "pvrtc_decode_device: out, pitch and blocks must be 4-byte aligned, "
				"pitch >= %zu", (size_t)width*4u);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		// no staging buffer is touched: the lease only carries the synchronisation rule of the stream
		StagingLease lease(ctx, call_stream(ctx, stream_));
		rc = pvrtc_decode_launch(ctx, format, blocks, width, height, out, out_pitch_bytes, nullptr, 0, nullptr, false,
			lease.stream);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

int cfhip_pvrtc_decode_sse(cfhip_ctx* ctx, int format, int type, const void* blocks, size_t blocks_bytes,
	uint32_t width, uint32_t height, const void* ref_rgba8, size_t ref_pitch_bytes, uint64_t sse[4])
{
	return guarded(ctx, "pvrtc_decode_sse", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		size_t payload = 0;
		int rc = pvrtc_decode_check(ctx, "pvrtc_decode_sse", format, type, blocks, width, height, &payload);
		if (rc != CFHIP_OK)
			return rc;
		if (!ref_rgba8 || !sse)
			return fail(ctx, CFHIP_E_INVALID, "pvrtc_decode_sse: NULL reference or result");
		if (blocks_bytes < payload)
			return fail(ctx, CFHIP_E_INVALID, "pvrtc_decode_sse: blocks_bytes %zu < %zu", blocks_bytes, payload);
		const size_t row = (size_t)width*4u;
		if (ref_pitch_bytes < row)
			return fail(ctx, CFHIP_E_INVALID, "pvrtc_decode_sse: reference pitch %zu < %zu", ref_pitch_bytes, row);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payload; d_out: the reference, tightly packed, then the four sums
		const size_t sum_off = (row*height + 15u) & ~(size_t)15u;
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, payload);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, sum_off + 32u);
		if (rc != CFHIP_OK)
			return rc;
		unsigned long long* d_sum = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(ctx->d_out) + sum_off);
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_src, blocks, payload, hipMemcpyHostToDevice, stream));
		HIP_TRY(ctx, hipMemcpy2DAsync(ctx->d_out, row, ref_rgba8, ref_pitch_bytes, row, height, hipMemcpyHostToDevice,
			stream));
		HIP_TRY(ctx, hipMemsetAsync(d_sum, 0, 32, stream));
		rc = pvrtc_decode_launch(ctx, format, ctx->d_src, width, height, nullptr, 0, ctx->d_out, row, d_sum, true, stream);
		if (rc != CFHIP_OK)
			return rc;
		unsigned long long sums[4] = {0, 0, 0, 0};
		HIP_TRY(ctx, hipMemcpyAsync(sums, d_sum, 32, hipMemcpyDeviceToHost, stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		for (int c = 0; c < 4; ++c)
			sse[c] = (uint64_t)sums[c];
		return CFHIP_OK;
	});
}

int cfhip_pvrtc_decode_sse_device(cfhip_ctx* ctx, int format, int type, const void* blocks, uint32_t width,
	uint32_t height, const void* ref_rgba8, size_t ref_pitch_bytes, uint64_t* sse_device, void* stream_)
{
	return guarded(ctx, "pvrtc_decode_sse_device", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		int rc = pvrtc_decode_check(ctx, "pvrtc_decode_sse_device", format, type, blocks, width, height, nullptr);
		if (rc != CFHIP_OK)
			return rc;
		if (!ref_rgba8 || !sse_device || ref_pitch_bytes < (size_t)width*4u || ((uintptr_t)ref_rgba8 & 3u) ||
			(ref_pitch_bytes & 3u) || ((uintptr_t)blocks & 3u))
			return fail(ctx, CFHIP_E_INVALID, "pvrtc_decode_sse_device: reference, pitch and blocks must be non-NULL and "
				"4-byte aligned, pitch >= %zu", (size_t)width*4u);
		// the kernel adds to the four sums with 64-bit atomics
		if ((uintptr_t)sse_device % 8u != 0)
			return fail(ctx, CFHIP_E_INVALID, "pvrtc_decode_sse_device: sse_device must be 8-byte aligned");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, call_stream(ctx, stream_));
		unsigned long long* sum = reinterpret_cast<unsigned long long*>(sse_device);
		HIP_TRY(ctx, hipMemsetAsync(sum, 0, 32, lease.stream));
		rc = pvrtc_decode_launch(ctx, format, blocks, width, height, nullptr, 0, ref_rgba8, ref_pitch_bytes, sum, true,
			lease.stream);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

} // extern "C"

// ---- standard formats 1..28 back to texels (csrc/std_unpack.hip) and their metrics (csrc/compare.hip) ----
struct StdGeom {
	int bpp;
	size_t payload_bytes;
};

// the checks every cfhip_std_* entry point makes before anything is enqueued
static int std_check(cfhip_ctx* ctx, const char* what, int format, int type, const void* pixels, uint32_t width,
	uint32_t height, StdGeom* g)
{
	g->bpp = is_std_format(format) ? std_pixel_bytes(format, type) : 0;
	if (!g->bpp)
		return fail(ctx, CFHIP_E_UNSUPPORTED, "%s: (format %d, type %d) is not a legal standard pair", what, format,
			type);
	if (!pixels)
		return fail(ctx, CFHIP_E_INVALID, "%s: pixels is NULL", what);
	if (!width || !height)
		return fail(ctx, CFHIP_E_INVALID, "%s: empty surface %ux%u", what, width, height);
	// one workgroup per 512 pixels in grid x
	if ((uint64_t)width*height > (1ull << 38))
		return fail(ctx, CFHIP_E_INVALID, "%s: surface %ux%u too large for one launch", what, width, height);
	g->payload_bytes = (size_t)width*height*(size_t)g->bpp;
	return CFHIP_OK;
}

// one unpack launch, timed like every encode launch (cfhip_last_kernel_ms / profiling)
static int std_unpack_launch(cfhip_ctx* ctx, int format, int type, const StdGeom& g, const void* pixels, void* out,
	size_t out_pitch, uint32_t width, uint32_t height, hipStream_t stream)
{
	begin_call(ctx, stream, "cfhip_std_unpack_kernel");
	return timed(ctx, stream, "std_unpack", [&] {
		return cfhip_launch_std_unpack(format, type, g.bpp, pixels, width, height, out, out_pitch, stream);
	});
}

// What one cfhip_std_compare call runs and where its device scratch lies: the unpacked surface of the SSIM pass
// (RGBA32F, tight), then the Pass A partials, then the SSIM partials.
struct StdCompareGeom {
	StdGeom g;
	int ref_bytes;
	unsigned cmask;
	bool hdr, ssim;
	uint64_t na, nb;
	uint32_t windows;
	size_t pa_off, pb_off, scratch_bytes;
};

// the channels a standard format stores, bit c = channel c
static unsigned std_channels(int format)
{
	switch (format) {
		case CFHIP_FORMAT_R8: case CFHIP_FORMAT_R16: case CFHIP_FORMAT_R32:
			return 1u;
		case CFHIP_FORMAT_R4G4: case CFHIP_FORMAT_R8G8: case CFHIP_FORMAT_R16G16: case CFHIP_FORMAT_R32G32:
			return 3u;
		case CFHIP_FORMAT_R5G6B5: case CFHIP_FORMAT_B5G6R5: case CFHIP_FORMAT_R8G8B8: case CFHIP_FORMAT_B8G8R8:
		case CFHIP_FORMAT_R16G16B16: case CFHIP_FORMAT_R32G32B32: case CFHIP_FORMAT_B10G11R11_UFLOAT:
		case CFHIP_FORMAT_E5B9G9R9_UFLOAT:
			return 7u;
		default:
			return 15u;
	}
}

static int std_compare_check(cfhip_ctx* ctx, const char* what, int format, int type, const void* pixels,
	uint32_t width, uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch, const uint8_t* mask,
	unsigned flags, const void* result, StdCompareGeom* c)
{
	int rc = std_check(ctx, what, format, type, pixels, width, height, &c->g);
	if (rc != CFHIP_OK)
		return rc;
	if (!ref || !result)
		return fail(ctx, CFHIP_E_INVALID, "%s: NULL reference or result", what);
	switch (ref_pixel_type) {
		case CFHIP_PIXEL_RGBA8: c->ref_bytes = 4; break;
		case CFHIP_PIXEL_RGBA32F: c->ref_bytes = 16; break;
		case CFHIP_PIXEL_RGBA16F: c->ref_bytes = 8; break;
		default: return fail(ctx, CFHIP_E_INVALID, "%s: reference pixel type %d", what, ref_pixel_type);
	}
	if (ref_pitch < (size_t)width*(size_t)c->ref_bytes)
		return fail(ctx, CFHIP_E_INVALID, "%s: reference pitch %zu < %zu", what, ref_pitch,
			(size_t)width*(size_t)c->ref_bytes);
	if (flags & ~CFHIP_COMPARE_SSIM)
		return fail(ctx, CFHIP_E_INVALID, "%s: unknown flags 0x%x", what, flags);
	unsigned m = 15u;
	if (mask)
		m = (mask[0] ? 1u : 0u) | (mask[1] ? 2u : 0u) | (mask[2] ? 4u : 0u) | (mask[3] ? 8u : 0u);
	c->cmask = std_channels(format) & m;
	c->hdr = type == CFHIP_TYPE_FLOAT || type == CFHIP_TYPE_UFLOAT;
	c->na = cfhip_std_compare_partials(width, height, &c->nb);
	const bool norm = type == CFHIP_TYPE_UNORM || type == CFHIP_TYPE_SNORM;
	c->ssim = (flags & CFHIP_COMPARE_SSIM) && norm && c->nb > 0 && c->cmask;
	if (!c->ssim)
		c->nb = 0;
	c->windows = 0;
	if (c->ssim) {
		const uint64_t win = (uint64_t)(width - 10u)*(height - 10u);
		if (win > 0xFFFFFFFFull || (height - 10u + 15u)/16u > 65535u)
			return fail(ctx, CFHIP_E_INVALID, "%s: surface %ux%u too large for SSIM", what, width, height);
		c->windows = (uint32_t)win;
	}
	const size_t dec = c->ssim ? (size_t)width*height*16u : 0;
	c->pa_off = align16(dec);
	c->pb_off = c->pa_off + (size_t)c->na*16u*sizeof(double);
	c->scratch_bytes = c->pb_off + (size_t)c->nb*4u*sizeof(double);
	return CFHIP_OK;
}

// Pass A, the SSIM pass (unpack into scratch + window statistics) and the final reduction, timed as one span
static int std_compare_enqueue(cfhip_ctx* ctx, int format, int type, const StdCompareGeom& c, const void* pixels,
	const void* ref, int ref_pixel_type, size_t ref_pitch, uint32_t width, uint32_t height, uint8_t* scratch,
	cfhip_compare_result* result, hipStream_t stream)
{
	begin_call(ctx, stream, "cfhip_std_compare_kernel");
	double* pa = reinterpret_cast<double*>(scratch + c.pa_off);
	double* pb = c.ssim ? reinterpret_cast<double*>(scratch + c.pb_off) : nullptr;
	return timed(ctx, stream, "std_compare", [&] {
		hipError_t e = cfhip_launch_std_compare(format, type, c.g.bpp, pixels, ref, ref_pixel_type, ref_pitch, width,
			height, c.cmask, c.hdr ? 1 : 0, pa, stream);
		if (e == hipSuccess && c.ssim) {
			const size_t dec_pitch = (size_t)width*16u;
			e = cfhip_launch_std_unpack(format, type, c.g.bpp, pixels, width, height, scratch, dec_pitch, stream);
			if (e == hipSuccess)
				e = cfhip_launch_ssim(scratch, dec_pitch, CFHIP_LAYOUT_RGBA32F, ref, ref_pixel_type, ref_pitch, width,
					height, c.cmask, ssim_taps(), type == CFHIP_TYPE_SNORM ? 2.0 : 1.0, pb, stream);
		}
		if (e == hipSuccess)
			e = cfhip_launch_compare_final(pa, c.na, pb, c.nb, c.cmask, c.hdr ? 1 : 0, c.windows,
				(uint64_t)width*height, result, stream);
		return e;
	});
}

extern "C" {

int cfhip_std_unpack(cfhip_ctx* ctx, int format, int type, const void* pixels, size_t pixels_bytes, uint32_t width,
	uint32_t height, void* out_rgba32f, size_t out_capacity)
{
	return guarded(ctx, "std_unpack", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		StdGeom g;
		int rc = std_check(ctx, "std_unpack", format, type, pixels, width, height, &g);
		if (rc != CFHIP_OK)
			return rc;
		if (!out_rgba32f)
			return fail(ctx, CFHIP_E_INVALID, "std_unpack: out is NULL");
		if (pixels_bytes < g.payload_bytes)
			return fail(ctx, CFHIP_E_INVALID, "std_unpack: pixels_bytes %zu < %zu for %ux%u", pixels_bytes,
				g.payload_bytes, width, height);
		const size_t out_bytes = (size_t)width*height*16u;
		if (out_capacity < out_bytes)
			return fail(ctx, CFHIP_E_CAPACITY, "std_unpack: out_capacity %zu < %zu", out_capacity, out_bytes);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payload; d_out: the texels
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, g.payload_bytes);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, out_bytes);
		if (rc != CFHIP_OK)
			return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_src, pixels, g.payload_bytes, hipMemcpyHostToDevice, stream));
		rc = std_unpack_launch(ctx, format, type, g, ctx->d_src, ctx->d_out, (size_t)width*16u, width, height, stream);
		if (rc != CFHIP_OK)
			return rc;
		HIP_TRY(ctx, hipMemcpyAsync(out_rgba32f, ctx->d_out, out_bytes, hipMemcpyDeviceToHost, stream));
		return lease.done(true);
	});
}

int cfhip_std_unpack_device(cfhip_ctx* ctx, int format, int type, const void* pixels, uint32_t width,
	uint32_t height, void* out_rgba32f, size_t out_pitch_bytes, void* stream_)
{
	return guarded(ctx, "std_unpack_device", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		StdGeom g;
		int rc = std_check(ctx, "std_unpack_device", format, type, pixels, width, height, &g);
		if (rc != CFHIP_OK)
			return rc;
		if (!out_rgba32f)
			return fail(ctx, CFHIP_E_INVALID, "std_unpack_device: out is NULL");
		if (out_pitch_bytes < (size_t)width*16u)
			return fail(ctx, CFHIP_E_INVALID, "std_unpack_device: out pitch %zu < %zu", out_pitch_bytes,
				(size_t)width*16u);
		// the kernel stores floats (whole float4 texels when pointer and pitch allow)
		if ((uintptr_t)out_rgba32f % 4u != 0 || out_pitch_bytes % 4u != 0)
			return fail(ctx, CFHIP_E_INVALID, "std_unpack_device: out and its pitch must be 4-byte aligned");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		// no staging buffer is touched: the lease only carries the synchronisation rule of the stream
		StagingLease lease(ctx, call_stream(ctx, stream_));
		rc = std_unpack_launch(ctx, format, type, g, pixels, out_rgba32f, out_pitch_bytes, width, height, lease.stream);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

int cfhip_std_compare(cfhip_ctx* ctx, int format, int type, const void* pixels, size_t pixels_bytes, uint32_t width,
	uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch_bytes, const uint8_t mask_rgba[4],
	unsigned flags, cfhip_compare_result* result)
{
	return guarded(ctx, "std_compare", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		StdCompareGeom c;
		int rc = std_compare_check(ctx, "std_compare", format, type, pixels, width, height, ref, ref_pixel_type,
			ref_pitch_bytes, mask_rgba, flags, result, &c);
		if (rc != CFHIP_OK)
			return rc;
		if (pixels_bytes < c.g.payload_bytes)
			return fail(ctx, CFHIP_E_INVALID, "std_compare: pixels_bytes %zu < %zu for %ux%u", pixels_bytes,
				c.g.payload_bytes, width, height);
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		StagingLease lease(ctx, ctx->stream);
		const hipStream_t stream = lease.stream;
		// d_src: the payload; d_out: the reference, tightly packed, the scratch, the result
		const size_t row = (size_t)width*(size_t)c.ref_bytes;
		const size_t scr_off = align16(row*height), res_off = align16(scr_off + c.scratch_bytes);
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_src, &ctx->src_cap, c.g.payload_bytes);
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, res_off + sizeof(cfhip_compare_result));
		if (rc != CFHIP_OK)
			return rc;
		uint8_t* d = static_cast<uint8_t*>(ctx->d_out);
		cfhip_compare_result* d_res = reinterpret_cast<cfhip_compare_result*>(d + res_off);
		HIP_TRY(ctx, hipMemcpyAsync(ctx->d_src, pixels, c.g.payload_bytes, hipMemcpyHostToDevice, stream));
		HIP_TRY(ctx, hipMemcpy2DAsync(d, row, ref, ref_pitch_bytes, row, height, hipMemcpyHostToDevice, stream));
		rc = std_compare_enqueue(ctx, format, type, c, ctx->d_src, d, ref_pixel_type, row, width, height, d + scr_off,
			d_res, stream);
		if (rc != CFHIP_OK)
			return rc;
		cfhip_compare_result res;
		HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, stream));
		rc = lease.done(true);
		if (rc != CFHIP_OK)
			return rc;
		*result = res;
		return CFHIP_OK;
	});
}

int cfhip_std_compare_device(cfhip_ctx* ctx, int format, int type, const void* pixels, uint32_t width,
	uint32_t height, const void* ref, int ref_pixel_type, size_t ref_pitch_bytes, const uint8_t mask_rgba[4],
	unsigned flags, cfhip_compare_result* result_device, void* stream_)
{
	return guarded(ctx, "std_compare_device", [&]() -> int {
		if (!ctx)
			return fail(nullptr, CFHIP_E_INVALID, "ctx is NULL");
		StdCompareGeom c;
		int rc = std_compare_check(ctx, "std_compare_device", format, type, pixels, width, height, ref, ref_pixel_type,
			ref_pitch_bytes, mask_rgba, flags, result_device, &c);
		if (rc != CFHIP_OK)
			return rc;
		// the kernels read reference texels with one aligned load each and store doubles to the result
		const size_t rb = (size_t)c.ref_bytes;
		if ((uintptr_t)ref % rb != 0 || ref_pitch_bytes % rb != 0)
			return fail(ctx, CFHIP_E_INVALID, "std_compare_device: reference and its pitch must be %zu-byte aligned", rb);
		if ((uintptr_t)result_device % 8u != 0)
			return fail(ctx, CFHIP_E_INVALID, "std_compare_device: misaligned result");
		HIP_TRY(ctx, hipSetDevice(ctx->device));
		// the partials (and the SSIM pass's unpacked surface) live in d_out: the lease orders them across streams
		StagingLease lease(ctx, call_stream(ctx, stream_));
		rc = lease.acquire();
		if (rc == CFHIP_OK)
			rc = reserve(ctx, &ctx->d_out, &ctx->out_cap, c.scratch_bytes);
		if (rc != CFHIP_OK)
			return rc;
		rc = std_compare_enqueue(ctx, format, type, c, pixels, ref, ref_pixel_type, ref_pitch_bytes, width, height,
			static_cast<uint8_t*>(ctx->d_out), result_device, lease.stream);
		if (rc != CFHIP_OK)
			return rc;
		return lease.done(!stream_);
	});
}

} // extern "C"

extern "C" {

float cfhip_last_kernel_ms(cfhip_ctx* ctx)
{
	if (!ctx)
		return -1.0f;
	std::lock_guard<std::mutex> guard(ctx->lock);
	if (!ctx->events_used)
		return -1.0f;
	if (hipSetDevice(ctx->device) != hipSuccess ||
		hipStreamSynchronize(ctx->events_stream) != hipSuccess)
		return -1.0f;
	float total = 0.0f;
	for (size_t i = 0; i + 1 < ctx->events_used; i += 2) {
		float ms = 0.0f;
		if (hipEventElapsedTime(&ms, ctx->events[i], ctx->events[i + 1]) != hipSuccess)
			return -1.0f;
		total += ms;
	}
	ctx->last_ms = total;
	return total;
}

int cfhip_profile_begin(cfhip_ctx* ctx)
{
	if (!ctx)
		return CFHIP_E_INVALID;
	std::lock_guard<std::mutex> guard(ctx->lock);
	ctx->profiling = true;
	ctx->events_used = 0;
	return CFHIP_OK;
}

int cfhip_profile_end(cfhip_ctx* ctx, float* total_ms, uint32_t* launches)
{
	if (!ctx)
		return CFHIP_E_INVALID;
	const float ms = cfhip_last_kernel_ms(ctx);
	std::lock_guard<std::mutex> guard(ctx->lock);
	ctx->profiling = false;
	if (total_ms) *total_ms = ms;
	if (launches) *launches = (uint32_t)(ctx->events_used/2);
	ctx->events_used = 0;
	return ms < 0.0f ? CFHIP_E_DEVICE : CFHIP_OK;
}

size_t cfhip_pinned_bytes(const cfhip_ctx* ctx)
{
	if (!ctx)
		return 0;
	size_t n = ctx->h_out ? ctx->h_out_cap : 0;
	for (int i = 0; i < cfhip_ctx::kPinSlots; ++i)
		n += ctx->h_pin[i] ? ctx->pin_cap : 0;
	return n;
}

const char* cfhip_last_kernel_name(const cfhip_ctx* ctx)
{
	return ctx ? ctx->last_kernel.c_str() : "";
}

const char* cfhip_last_error(const cfhip_ctx* ctx)
{
	if (ctx)
		return ctx->error.c_str();
	return g_error.c_str();
}

} // extern "C"
