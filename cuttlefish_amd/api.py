"""ctypes binding of the C-ABI in include/cuttlefish_hip.h (libcuttlefish_hip.so).

This is plumbing: the product is the HIP library.  There is no CPU fallback --
if the library or a HIP device is missing every call raises.
"""
from __future__ import annotations

import ctypes
import enum
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libcuttlefish_hip.so")


class Format(enum.IntEnum):
    """cuttlefish::Texture::Format values (lib/include/cuttlefish/Texture.h:59-130)."""
    R4G4 = 1
    R4G4B4A4 = 2
    B4G4R4A4 = 3
    A4R4G4B4 = 4
    R5G6B5 = 5
    B5G6R5 = 6
    R5G5B5A1 = 7
    B5G5R5A1 = 8
    A1R5G5B5 = 9
    R8 = 10
    R8G8 = 11
    R8G8B8 = 12
    B8G8R8 = 13
    R8G8B8A8 = 14
    B8G8R8A8 = 15
    A8B8G8R8 = 16
    A2R10G10B10 = 17
    A2B10G10R10 = 18
    R16 = 19
    R16G16 = 20
    R16G16B16 = 21
    R16G16B16A16 = 22
    R32 = 23
    R32G32 = 24
    R32G32B32 = 25
    R32G32B32A32 = 26
    B10G11R11_UFloat = 27
    E5B9G9R9_UFloat = 28
    BC1_RGB = 29
    BC1_RGBA = 30
    BC2 = 31
    BC3 = 32
    BC4 = 33
    BC5 = 34
    BC6H = 35
    BC7 = 36
    ETC1 = 37
    ETC2_R8G8B8 = 38
    ETC2_R8G8B8A1 = 39
    ETC2_R8G8B8A8 = 40
    EAC_R11 = 41
    EAC_R11G11 = 42
    ASTC_4x4 = 43
    ASTC_5x4 = 44
    ASTC_5x5 = 45
    ASTC_6x5 = 46
    ASTC_6x6 = 47
    ASTC_8x5 = 48
    ASTC_8x6 = 49
    ASTC_8x8 = 50
    ASTC_10x5 = 51
    ASTC_10x6 = 52
    ASTC_10x8 = 53
    ASTC_10x10 = 54
    ASTC_12x10 = 55
    ASTC_12x12 = 56
    # PVRTC (Texture.h:124-129): query() still raises for all six; PVRTC1 4 bpp goes through pvrtc_payload_size and
    # the Context.*_pvrtc calls, the 2 bpp and PVRTC2 formats are not built
    PVRTC1_RGB_2BPP = 57
    PVRTC1_RGBA_2BPP = 58
    PVRTC1_RGB_4BPP = 59
    PVRTC1_RGBA_4BPP = 60
    PVRTC2_RGBA_2BPP = 61
    PVRTC2_RGBA_4BPP = 62


PVRTC_FORMATS = (Format.PVRTC1_RGB_4BPP, Format.PVRTC1_RGBA_4BPP)


class Type(enum.IntEnum):
    """cuttlefish::Texture::Type (Texture.h:135-143)."""
    UNorm = 0
    SNorm = 1
    UInt = 2
    Int = 3
    UFloat = 4
    Float = 5


class Quality(enum.IntEnum):
    """cuttlefish::Texture::Quality (Texture.h:181-188)."""
    Lowest = 0
    Low = 1
    Normal = 2
    High = 3
    Highest = 4


class Alpha(enum.IntEnum):
    """cuttlefish::Texture::Alpha (Texture.h:161-167)."""
    None_ = 0
    Standard = 1
    PreMultiplied = 2
    Encoded = 3


class ColorSpace(enum.IntEnum):
    """cuttlefish::ColorSpace (Color.h:40-44)."""
    Linear = 0
    sRGB = 1


class ResizeFilter(enum.IntEnum):
    """cuttlefish::Image::ResizeFilter (Image.h:79-86)."""
    Box = 0
    Linear = 1
    Cubic = 2
    CatmullRom = 3
    BSpline = 4


class Channel(enum.IntEnum):
    """cuttlefish::Image::Channel (Image.h:104-111)."""
    Red = 0
    Green = 1
    Blue = 2
    Alpha = 3
    None_ = 4


class RotateAngle(enum.IntEnum):
    """cuttlefish::Image::RotateAngle (Image.h:91-99)."""
    CW90 = 0
    CW180 = 1
    CW270 = 2
    CCW90 = 3
    CCW180 = 4
    CCW270 = 5


class NormalOptions(enum.IntFlag):
    """cuttlefish::Image::NormalOptions (Image.h:116-122), a bit mask."""
    Default = 0
    KeepSign = 1
    WrapX = 2
    WrapY = 4


class ImageOp(enum.IntFlag):
    """The op bits of ImageOps.ops (enum cfhip_image_op); a call runs them in this order."""
    ColorSpace = 1 << 0
    Rotate = 1 << 1
    Grayscale = 1 << 2
    NormalMap = 1 << 3
    FlipX = 1 << 4
    FlipY = 1 << 5
    Swizzle = 1 << 6
    PreMultiply = 1 << 7


class PixelType(enum.IntEnum):
    RGBA8 = 0
    RGBA32F = 1
    RGBA16F = 2


E_INVALID, E_UNSUPPORTED, E_CAPACITY, E_DEVICE, E_NO_DEVICE = -1, -2, -3, -4, -5
E_DATA = -6                     # cfhip_inflate: the stream or its index is invalid

# cfhip_consumed_fn: void (*)(void* user, size_t surface_index)
CONSUMED_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_size_t)

EXPORTS = ["cfhip_abi_version", "cfhip_device_count", "cfhip_create", "cfhip_destroy",
           "cfhip_query", "cfhip_encode", "cfhip_encode_multi", "cfhip_encode_multi_ex", "cfhip_encode_device",
           "cfhip_shard_rows",
           "cfhip_last_kernel_ms", "cfhip_last_kernel_name", "cfhip_last_error", "cfhip_pinned_bytes",
           "cfhip_profile_begin", "cfhip_profile_end", "cfhip_generate_mips_device",
           "cfhip_generate_mips3d_device", "cfhip_resize_device", "cfhip_generate_mips_array_device",
           "cfhip_decoded_layout", "cfhip_decode", "cfhip_decode_device", "cfhip_decode_sse",
           "cfhip_decode_sse_device", "cfhip_image_ops_device", "cfhip_compare", "cfhip_compare_device",
           "cfhip_pvrtc_query", "cfhip_pvrtc_encode", "cfhip_pvrtc_encode_device", "cfhip_pvrtc_decode",
           "cfhip_pvrtc_decode_device", "cfhip_pvrtc_decode_sse", "cfhip_pvrtc_decode_sse_device",
           "cfhip_std_unpack", "cfhip_std_unpack_device", "cfhip_std_compare", "cfhip_std_compare_device",
           "cfhip_decode_batch", "cfhip_decode_batch_device", "cfhip_decode_out_supported",
           "cfhip_compare_batch", "cfhip_compare_batch_device",
           "cfhip_rdo_supported", "cfhip_rdo", "cfhip_rdo_device",
           "cfhip_rdo_ex", "cfhip_rdo_ex_device",
           "cfhip_lz_size", "cfhip_lz_size_device", "cfhip_lz_slice_bytes", "cfhip_lz_stage_ms",
           "cfhip_rdo_target", "cfhip_rdo_target_device",
           "cfhip_deflate_bound", "cfhip_deflate", "cfhip_deflate_device", "cfhip_deflate_stage_ms",
           "cfhip_deflate_code_lengths",
           "cfhip_zindex_entries", "cfhip_deflate_indexed", "cfhip_deflate_indexed_device",
           "cfhip_inflate", "cfhip_inflate_device", "cfhip_inflate_stage_ms",
           "cfhip_lz4_bound", "cfhip_lz4_encode", "cfhip_lz4_encode_device", "cfhip_lz4_encode_stage_ms",
           "cfhip_lz4_decode", "cfhip_lz4_decode_device", "cfhip_lz4_decode_stage_ms",
           "cfhip_png_bound", "cfhip_png_encode", "cfhip_png_encode_device", "cfhip_png_stage_ms",
           "cfhip_mip_post_array_device", "cfhip_alpha_coverage_device", "cfhip_alpha_bleed_array_device",
           "cfhip_alpha_sdf_array_device", "cfhip_spec_aa_array_device",
           "cfhip_height_ao_array_device", "cfhip_height_ao_directions",
           "cfhip_equirect_to_cube_device", "cfhip_ggx_sample_table", "cfhip_cube_prefilter_device",
           "cfhip_cube_sh9_device",
           "cfhip_lobe_sample_table", "cfhip_hammersley_table", "cfhip_brdf_lut_device", "cfhip_cube_irradiance_device"]


class Layout(enum.IntEnum):
    """Decoded texel layouts (enum cfhip_layout)."""
    RGBA8 = 0
    R8 = 1
    R8_SNorm = 2
    RG8 = 3
    RG8_SNorm = 4
    R16 = 5
    R16_SNorm = 6
    RG16 = 7
    RG16_SNorm = 8
    RGBA16F = 9
    RGBA32F = 10                # what Context.unpack returns for the standard formats


# layout -> (channels, numpy dtype) of the decoded array
LAYOUT_ARRAY = {Layout.RGBA8: (4, np.uint8), Layout.R8: (1, np.uint8), Layout.R8_SNorm: (1, np.int8),
                Layout.RG8: (2, np.uint8), Layout.RG8_SNorm: (2, np.int8), Layout.R16: (1, np.uint16),
                Layout.R16_SNorm: (1, np.int16), Layout.RG16: (2, np.uint16), Layout.RG16_SNorm: (2, np.int16),
                Layout.RGBA16F: (4, np.float16), Layout.RGBA32F: (4, np.float32)}

COMPARE_SSIM = 1                # CFHIP_COMPARE_SSIM


class CompareResult(ctypes.Structure):
    """struct cfhip_compare_result."""
    _fields_ = [("texels", ctypes.c_uint64), ("error_blocks", ctypes.c_uint64), ("channels", ctypes.c_uint32),
                ("ssim_windows", ctypes.c_uint32), ("sse", ctypes.c_double * 4), ("log_sse", ctypes.c_double * 4),
                ("ssim", ctypes.c_double * 4), ("ref_max", ctypes.c_double * 4)]


class Comparison:
    """What Context.compare returns: the metrics of one surface (cfhip_compare_result) and, when asked, the
    (blocks_y, blocks_x) float32 map of per-block SSE."""

    def __init__(self, res: CompareResult, layout: Layout, block_errors: Optional[np.ndarray] = None, typ=None):
        self.layout = Layout(layout)
        self.type = None if typ is None else Type(typ)      # set for the standard formats (layout RGBA32F)
        self.texels = int(res.texels)
        self.error_blocks = int(res.error_blocks)
        self.channels = int(res.channels)
        self.ssim_windows = int(res.ssim_windows)
        self.sse = [float(v) for v in res.sse]
        self.log_sse = [float(v) for v in res.log_sse]
        self.ssim = [float(v) for v in res.ssim]
        self.ref_max = [float(v) for v in res.ref_max]
        self.block_errors = block_errors

    def compared(self):
        """Indices of the compared channels."""
        return [c for c in range(4) if (self.channels >> c) & 1]

    def peak(self, channels=None) -> float:
        """The data range: 1 for UNorm layouts, 2 for SNorm layouts, the largest reference value for HDR.  Standard
        formats: 1 for UNorm, 2 for SNorm, the largest reference value of the compared channels for the other
        types."""
        if self.layout == Layout.RGBA32F and self.type in (Type.UNorm, Type.SNorm):
            return 2.0 if self.type == Type.SNorm else 1.0
        if self.layout in (Layout.RGBA16F, Layout.RGBA32F):
            chans = self.compared() if channels is None else list(channels)
            return max(self.ref_max[c] for c in chans)
        return 2.0 if self.layout.name.endswith("SNorm") else 1.0

    def psnr(self, channels=None, peak=None) -> float:
        """PSNR (dB) over `channels` (default: the compared ones); peak defaults to the data range."""
        chans = self.compared() if channels is None else list(channels)
        if not chans:
            raise ValueError("no channel to measure")
        total = sum(self.sse[c] for c in chans)
        if total == 0.0:
            return float("inf")
        p = self.peak(chans) if peak is None else float(peak)
        return 10.0 * float(np.log10(p * p * self.texels * len(chans) / total))


class Params(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("type", ctypes.c_int32), ("quality", ctypes.c_int32),
                ("alpha", ctypes.c_int32), ("mask_rgba", ctypes.c_uint8 * 4),
                ("color_space", ctypes.c_int32)]


class Surface(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_void_p), ("pixel_type", ctypes.c_int32),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("row_pitch_bytes", ctypes.c_ssize_t), ("out", ctypes.c_void_p),
                ("out_capacity", ctypes.c_size_t)]


class DecodeSurface(ctypes.Structure):
    """struct cfhip_decode_surface"""
    _fields_ = [("blocks", ctypes.c_void_p), ("blocks_bytes", ctypes.c_size_t), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("out", ctypes.c_void_p), ("out_pitch_bytes", ctypes.c_size_t),
                ("out_capacity", ctypes.c_size_t)]


class CompareSurface(ctypes.Structure):
    """struct cfhip_compare_surface"""
    _fields_ = [("blocks", ctypes.c_void_p), ("blocks_bytes", ctypes.c_size_t), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("ref", ctypes.c_void_p), ("ref_pitch_bytes", ctypes.c_size_t),
                ("block_errors", ctypes.c_void_p), ("block_errors_capacity", ctypes.c_size_t)]


class RdoParams(ctypes.Structure):
    """struct cfhip_rdo_params"""
    _fields_ = [("lam", ctypes.c_float), ("max_sse_increase", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class RdoExParams(ctypes.Structure):
    """struct cfhip_rdo_ex_params"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("lam", ctypes.c_float), ("max_sse_increase", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("window_bytes", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class RdoSurface(ctypes.Structure):
    """struct cfhip_rdo_surface"""
    _fields_ = [("blocks", ctypes.c_void_p), ("blocks_bytes", ctypes.c_size_t), ("out", ctypes.c_void_p),
                ("out_capacity", ctypes.c_size_t), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("pixels", ctypes.c_void_p), ("pixel_type", ctypes.c_int32), ("row_pitch_bytes", ctypes.c_size_t)]


class RdoStats(ctypes.Structure):
    """struct cfhip_rdo_stats"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("blocks", "blocks_changed", "sse_before", "sse_after", "bits_before",
                                               "bits_after")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class LzSpan(ctypes.Structure):
    """struct cfhip_lz_span"""
    _fields_ = [("bytes", ctypes.c_void_p), ("n", ctypes.c_size_t)]


class LzStats(ctypes.Structure):
    """struct cfhip_lz_stats"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("bytes_in", "bits_q16", "est_bytes", "literals", "matches",
                                               "matched_bytes")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RdoTargetResult(ctypes.Structure):
    """struct cfhip_rdo_target_result"""
    _fields_ = [("lambda16", ctypes.c_uint32), ("reached", ctypes.c_uint32), ("trials", ctypes.c_uint32),
                ("est_bytes_plain", ctypes.c_uint64), ("est_bytes_final", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


LZ_STAGES = ("keys", "sort", "match", "parse", "cost")      # cfhip_lz_stage_ms


class DeflateResult(ctypes.Structure):
    """struct cfhip_deflate_result"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("bytes_in", "bytes_out", "blocks_stored", "blocks_fixed",
                                               "blocks_dynamic", "literals", "matches", "matched_bytes")] + \
               [("adler32", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


DEFLATE_STAGES = ("keys", "sort", "match", "parse", "adler", "codes", "offsets", "emit")   # cfhip_deflate_stage_ms


def deflate_bound(n: int) -> int:
    """cfhip_deflate_bound: bytes that hold the zlib stream of any n input bytes (no device needed)"""
    return int(load_library().cfhip_deflate_bound(int(n)))



class ZIndexEntry(ctypes.Structure):
    """struct cfhip_zindex_entry"""
    _fields_ = [("header_bit", ctypes.c_uint64), ("token_bit", ctypes.c_uint64)]


class InflateResult(ctypes.Structure):
    """struct cfhip_inflate_result"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("bytes_in", "bytes_out", "literals", "matches", "matched_bytes")] + \
               [(n, ctypes.c_uint32) for n in ("adler32", "status", "bad_chunk", "rounds")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


INFLATE_STAGES = ("decode", "resolve", "pack", "fold")      # cfhip_inflate_stage_ms
# enum cfhip_inflate_status
INFLATE_CLASSES = ("ok", "wrapper", "index", "block header", "code", "distance", "overrun", "checksum")
ZINDEX_CHUNK = 4096             # output bytes per index entry


def zindex_entries(n: int) -> int:
    """cfhip_zindex_entries: entries of the index of a stream whose output is n bytes (no device needed)"""
    return int(load_library().cfhip_zindex_entries(int(n)))


class Lz4Result(ctypes.Structure):
    """struct cfhip_lz4_result"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("bytes_in", "bytes_out", "blocks_compressed", "blocks_stored", "sequences",
                                               "literals", "matched_bytes")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Lz4DecodeResult(ctypes.Structure):
    """struct cfhip_lz4_decode_result"""
    _fields_ = Lz4Result._fields_ + [(n, ctypes.c_uint32) for n in ("status", "bad_block", "content_checksum", "reserved")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


LZ4_ENCODE_STAGES = ("keys", "sort", "match", "parse", "plan", "offsets", "emit", "hash", "final")   # cfhip_lz4_encode_stage_ms
LZ4_DECODE_STAGES = ("chain", "blocks", "final")                                                     # cfhip_lz4_decode_stage_ms
# enum cfhip_lz4_status
LZ4_CLASSES = ("ok", "header", "unsupported", "blocks", "checksum", "sequence", "offset", "size")
LZ4_UNSUPPORTED = 2             # a valid frame this decoder does not take: decode it on the host
LZ4_BLOCK = 65536               # input bytes per block
LZ4_MAGIC = b"\x04\x22\x4D\x18"


def lz4_bound(n: int) -> int:
    """cfhip_lz4_bound: bytes that hold the LZ4 frame of any n input bytes (no device needed)"""
    return int(load_library().cfhip_lz4_bound(int(n)))


class PngResult(ctypes.Structure):
    """struct cfhip_png_result"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("bytes_out", "idat_bytes", "filtered_bytes")] + \
               [("rows_by_filter", ctypes.c_uint32*5), ("idat_crc32", ctypes.c_uint32), ("deflate", DeflateResult)]

    def as_dict(self) -> dict:
        return {"bytes_out": int(self.bytes_out), "idat_bytes": int(self.idat_bytes),
                "filtered_bytes": int(self.filtered_bytes), "rows_by_filter": [int(v) for v in self.rows_by_filter],
                "idat_crc32": int(self.idat_crc32), "deflate": self.deflate.as_dict()}


PNG_STAGES = ("filter",) + DEFLATE_STAGES + ("crc", "final")       # cfhip_png_stage_ms
PNG_GREY, PNG_RGB, PNG_GREY_ALPHA, PNG_RGBA = 0, 2, 4, 6           # the colour types written
PNG_FILTERS = ("none", "sub", "up", "average", "paeth")            # cfhip_png_result.rows_by_filter


def png_bound(width: int, height: int, color_type: int = PNG_RGBA, bit_depth: int = 8, color_space=0) -> int:
    """cfhip_png_bound: bytes that hold the PNG file of any such image (no device needed); 0 for an image
    cfhip_png_encode does not take"""
    return int(load_library().cfhip_png_bound(int(width), int(height), int(color_type), int(bit_depth), int(color_space)))


MIP_POST_COVERAGE, MIP_POST_NORMALIZE, MIP_POST_SIGNED_NORMALS = 1, 2, 4     # cfhip_mip_post_params.flags


class MipPostParams(ctypes.Structure):
    """cfhip_mip_post_params"""
    _fields_ = [("flags", ctypes.c_uint32), ("alpha_threshold", ctypes.c_float)]


class MipPostResult(ctypes.Structure):
    """cfhip_mip_post_result: one generated level's scale, its target count and its counts at scale 1 and at the scale"""
    _fields_ = [("scale", ctypes.c_float), ("target", ctypes.c_uint32), ("count_before", ctypes.c_uint32),
                ("count_after", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {"scale": float(self.scale), "target": int(self.target), "count_before": int(self.count_before),
                "count_after": int(self.count_after)}


MIP_POST_RESULT_DTYPE = np.dtype([("scale", np.float32), ("target", np.uint32), ("count_before", np.uint32),
                                  ("count_after", np.uint32)])


class CoverageSurface(ctypes.Structure):
    """cfhip_coverage_surface"""
    _fields_ = [("pixels", ctypes.c_void_p), ("pixel_type", ctypes.c_int32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("pitch_bytes", ctypes.c_size_t)]


def make_mip_post_params(alpha_coverage: Optional[float] = None, normalize: Optional[str] = None) -> MipPostParams:
    """alpha_coverage: the alpha-test threshold in (0, 1], or None; normalize: "unorm" (Image.create_normal_map's
    storage without KEEP_SIGN), "snorm" (signed storage) or None."""
    if normalize not in (None, "unorm", "snorm"):
        raise ValueError('normalize is "unorm", "snorm" or None, not %r' % (normalize,))
    flags = (MIP_POST_COVERAGE if alpha_coverage is not None else 0) | (MIP_POST_NORMALIZE if normalize else 0) | \
        (MIP_POST_SIGNED_NORMALS if normalize == "snorm" else 0)
    return MipPostParams(flags, float(alpha_coverage) if alpha_coverage is not None else 0.0)


BLEED_WRAP_X, BLEED_WRAP_Y = 1, 2                # cfhip_bleed_params.flags


class BleedParams(ctypes.Structure):
    """cfhip_bleed_params"""
    _fields_ = [("flags", ctypes.c_uint32), ("alpha_threshold", ctypes.c_float), ("max_distance", ctypes.c_uint32)]


class BleedResult(ctypes.Structure):
    """cfhip_bleed_result: one surface's seeds, its filled texels and the largest squared distance a colour travelled"""
    _fields_ = [("seeds", ctypes.c_uint32), ("filled", ctypes.c_uint32), ("max_dist2", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


BLEED_RESULT_DTYPE = np.dtype([("seeds", np.uint32), ("filled", np.uint32), ("max_dist2", np.uint32),
                               ("reserved", np.uint32)])


def wrap_axes(wrap) -> Tuple[bool, bool]:
    """wrap as the bleed methods take it: one bool for both axes, or (x, y)"""
    if isinstance(wrap, (bool, np.bool_)):
        return bool(wrap), bool(wrap)
    x, y = wrap
    return bool(x), bool(y)


def make_bleed_params(threshold: float = 0.0, wrap=(False, False), max_distance: int = 0) -> BleedParams:
    """threshold: texels with alpha > threshold are the seeds (0 <= threshold < 1); wrap: a bool or (x, y), the axes
    on which the surface tiles; max_distance: how far a colour may travel in texels, 0 = unlimited.  Ranges are the
    library's to check."""
    wx, wy = wrap_axes(wrap)
    return BleedParams((BLEED_WRAP_X if wx else 0) | (BLEED_WRAP_Y if wy else 0), float(threshold), int(max_distance))


SDF_WRAP_X, SDF_WRAP_Y = 1, 2                    # cfhip_sdf_params.flags
SDF_SCALES = (1, 2, 4, 8, 16)
SDF_MAX_SPREAD = 126
SDF_CHANNELS = {"r": 1, "g": 2, "b": 4, "a": 8}   # cfhip_sdf_params.channel_mask


class SdfParams(ctypes.Structure):
    """cfhip_sdf_params"""
    _fields_ = [("flags", ctypes.c_uint32), ("alpha_threshold", ctypes.c_float), ("spread", ctypes.c_uint32),
                ("scale", ctypes.c_uint32), ("channel_mask", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class SdfResult(ctypes.Structure):
    """cfhip_sdf_result: one surface's source texels inside, and those farther than the spread from the silhouette"""
    _fields_ = [("inside", ctypes.c_uint32), ("saturated", ctypes.c_uint32), ("reserved", ctypes.c_uint32*2)]


SDF_RESULT_DTYPE = np.dtype([("inside", np.uint32), ("saturated", np.uint32), ("reserved0", np.uint32),
                             ("reserved1", np.uint32)])


def sdf_channel_mask(channels) -> int:
    """channels as the distance-field methods take them: a string of r, g, b, a (any case, each at most once) or the
    mask itself (R = 1, G = 2, B = 4, A = 8)"""
    if isinstance(channels, (int, np.integer)) and not isinstance(channels, (bool, np.bool_)):
        mask = int(channels)
    elif isinstance(channels, str) and channels:
        mask = 0
        for ch in channels.lower():
            if ch not in SDF_CHANNELS or mask & SDF_CHANNELS[ch]:
                raise ValueError("channels %r: a string of r, g, b, a, each at most once" % (channels,))
            mask |= SDF_CHANNELS[ch]
    else:
        raise ValueError("channels %r: a string of r, g, b, a, or a mask of 1 to 15" % (channels,))
    if not 1 <= mask <= 15:
        raise ValueError("channels %r: a mask of 1 to 15" % (channels,))
    return mask


def make_sdf_params(spread: int, scale: int = 1, threshold: float = 0.5, wrap=(False, False), channels="a") -> SdfParams:
    """spread: the distance in source texels at which the field reaches 0 and 1 (1 to 126); scale: source texels per
    output texel and side (1, 2, 4, 8 or 16); threshold: texels with alpha > threshold are inside (0 <= threshold < 1);
    wrap: a bool or (x, y), the axes on which the surface tiles; channels: the components that receive the field.
    Every bad field is a ValueError here, before the library would refuse it."""
    if isinstance(spread, (bool, np.bool_)) or not isinstance(spread, (int, np.integer)) or not 1 <= spread <= SDF_MAX_SPREAD:
        raise ValueError("spread %r: an integer from 1 to %d" % (spread, SDF_MAX_SPREAD))
    if isinstance(scale, (bool, np.bool_)) or scale not in SDF_SCALES:
        raise ValueError("scale %r: one of %r" % (scale, SDF_SCALES))
    t = float(threshold)
    if not 0.0 <= t < 1.0 or not 0.0 <= float(np.float32(t)) < 1.0:
        raise ValueError("threshold %r outside [0, 1)" % (threshold,))
    wx, wy = wrap_axes(wrap)
    return SdfParams((SDF_WRAP_X if wx else 0) | (SDF_WRAP_Y if wy else 0), t, int(spread), int(scale),
                     sdf_channel_mask(channels), 0)


SPEC_AA_PERCEPTUAL, SPEC_AA_SIGNED_NORMALS, SPEC_AA_RECONSTRUCT_Z = 1, 2, 4      # cfhip_spec_aa_params.flags
SPEC_AA_CHANNELS = {"r": 0, "g": 1, "b": 2, "a": 3}                               # cfhip_spec_aa_params.channel


class SpecAaParams(ctypes.Structure):
    """cfhip_spec_aa_params"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("channel", ctypes.c_uint32),
                ("base_roughness", ctypes.c_float), ("variance_scale", ctypes.c_float), ("max_variance", ctypes.c_float),
                ("reserved", ctypes.c_uint32*2)]


class SpecAaResult(ctypes.Structure):
    """cfhip_spec_aa_result: one level's texels whose variance met max_variance, those whose alpha^2 reached 1, and the
    bit pattern of the largest (float)(variance_scale * v) added"""
    _fields_ = [("clamped", ctypes.c_uint32), ("saturated", ctypes.c_uint32), ("max_added", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


SPEC_AA_RESULT_DTYPE = np.dtype([("clamped", np.uint32), ("saturated", np.uint32), ("max_added", np.uint32),
                                 ("reserved", np.uint32)])


def spec_aa_channel(channel) -> int:
    """channel as the specular anti-aliasing methods take it: one of "r", "g", "b", "a" (any case) or 0 to 3"""
    if isinstance(channel, str) and channel.lower() in SPEC_AA_CHANNELS:
        return SPEC_AA_CHANNELS[channel.lower()]
    if isinstance(channel, (int, np.integer)) and not isinstance(channel, (bool, np.bool_)) and 0 <= channel <= 3:
        return int(channel)
    raise ValueError('channel %r: one of "r", "g", "b", "a" or 0 to 3' % (channel,))


def make_spec_aa_params(channel, perceptual: bool = True, signed_normals: bool = False, reconstruct_z: bool = False,
                        base_roughness: float = 0.5, variance_scale: float = 1.0,
                        max_variance: float = 1.0) -> SpecAaParams:
    """channel: the component of the roughness chain that is rewritten; perceptual: the stored value is perceptual
    roughness (alpha = r^2), else alpha itself; signed_normals: the normals are stored as they are, else as n/2 + 1/2;
    reconstruct_z: two-channel normals, z from x and y; base_roughness: every texel's roughness when there is no
    level-0 roughness map; variance_scale, max_variance: 1 and 1 are the plain vMF form, 2 and 0.18 the clamp of
    Kaplanyan et al.  Every bad field is a ValueError here, before the library would refuse it."""
    with np.errstate(over="ignore"):                   # a value beyond float32 becomes inf and is refused below
        b, s, m = (float(np.float32(v)) for v in (base_roughness, variance_scale, max_variance))
    if not 0.0 <= b <= 1.0:
        raise ValueError("base_roughness %r outside [0, 1]" % (base_roughness,))
    if not (s >= 0.0 and np.isfinite(s)):
        raise ValueError("variance_scale %r is negative or not finite" % (variance_scale,))
    if not (m >= 0.0 and np.isfinite(m)):
        raise ValueError("max_variance %r is negative or not finite" % (max_variance,))
    flags = (SPEC_AA_PERCEPTUAL if perceptual else 0) | (SPEC_AA_SIGNED_NORMALS if signed_normals else 0) | \
        (SPEC_AA_RECONSTRUCT_Z if reconstruct_z else 0)
    return SpecAaParams(ctypes.sizeof(SpecAaParams), flags, spec_aa_channel(channel), b, s, m, (ctypes.c_uint32*2)(0, 0))


# ---- ambient occlusion from height maps (cfhip_height_ao_array_device) ----
HAO_WRAP_X, HAO_WRAP_Y, HAO_UNIFORM, HAO_FALLOFF = 1, 2, 4, 8      # cfhip_height_ao_params.flags
HAO_DIRECTIONS = (8, 16, 32)
HAO_MAX_RADIUS = 64


class HeightAoParams(ctypes.Structure):
    """cfhip_height_ao_params"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("channel", ctypes.c_uint32),
                ("directions", ctypes.c_uint32), ("radius", ctypes.c_uint32), ("channel_mask", ctypes.c_uint32),
                ("height", ctypes.c_float), ("strength", ctypes.c_float), ("bias", ctypes.c_float),
                ("reserved", ctypes.c_uint32)]


class HeightAoResult(ctypes.Structure):
    """cfhip_height_ao_result: one surface's texels with a horizon above the bias in any direction, and the bit pattern
    of its smallest (float)v"""
    _fields_ = [("occluded", ctypes.c_uint32), ("darkest", ctypes.c_uint32), ("reserved", ctypes.c_uint32*2)]


HEIGHT_AO_RESULT_DTYPE = np.dtype([("occluded", np.uint32), ("darkest", np.uint32), ("reserved0", np.uint32),
                                   ("reserved1", np.uint32)])


def make_height_ao_params(radius: int, height_scale: float = 1.0, directions: int = 16, channel="r", channels="r",
                          strength: float = 1.0, bias: float = 0.0, uniform: bool = False, falloff: bool = False,
                          wrap=(False, False)) -> HeightAoParams:
    """radius: how far a horizon is looked for, in texels (1 to 64); height_scale: texels per stored unit of height, the
    meaning the normal-map op's height has (finite, negative for an inverted map); directions: 8, 16 or 32; channel:
    the component that holds the height; channels: the components that receive the occlusion; strength: 1 is the
    occlusion itself, 0 none, above 1 darker (clamped at 0); bias: the slope a horizon must exceed to count; uniform:
    solid-angle visibility instead of the cosine-weighted one; falloff: a horizon's slope fades to 0 at radius + 1;
    wrap: a bool or (x, y), the axes on which the surface tiles.  Every bad field is a ValueError here, before the
    library would refuse it."""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= HAO_MAX_RADIUS:
        raise ValueError("radius %r: an integer from 1 to %d" % (radius, HAO_MAX_RADIUS))
    if isinstance(directions, (bool, np.bool_)) or directions not in HAO_DIRECTIONS:
        raise ValueError("directions %r: one of %r" % (directions, HAO_DIRECTIONS))
    with np.errstate(over="ignore"):                   # a value beyond float32 becomes inf and is refused below
        hs, s, b = (float(np.float32(v)) for v in (height_scale, strength, bias))
    if not np.isfinite(hs):
        raise ValueError("height_scale %r is not finite" % (height_scale,))
    if not (s >= 0.0 and np.isfinite(s)):
        raise ValueError("strength %r is negative or not finite" % (strength,))
    if not (b >= 0.0 and np.isfinite(b)):
        raise ValueError("bias %r is negative or not finite" % (bias,))
    wx, wy = wrap_axes(wrap)
    flags = (HAO_WRAP_X if wx else 0) | (HAO_WRAP_Y if wy else 0) | (HAO_UNIFORM if uniform else 0) | \
        (HAO_FALLOFF if falloff else 0)
    return HeightAoParams(ctypes.sizeof(HeightAoParams), flags, spec_aa_channel(channel), int(directions), int(radius),
                          sdf_channel_mask(channels), hs, s, b, 0)


def height_ao_directions(D: int):
    """cfhip_height_ao_directions -> (vx, vy, weight): the D (8, 16 or 32) integer direction vectors of the horizon scan
    as int32 arrays and each one's share of the circle as float64.  Host only: no context, no device."""
    if isinstance(D, (bool, np.bool_)) or D not in HAO_DIRECTIONS:
        raise ValueError("directions %r: one of %r" % (D, HAO_DIRECTIONS))
    vx, vy, w = np.empty(D, np.int32), np.empty(D, np.int32), np.empty(D, np.float64)
    rc = load_library().cfhip_height_ao_directions(int(D), vx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                   vy.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                   w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if rc != 0:
        raise ValueError("cfhip_height_ao_directions refused %r" % (D,))
    return vx, vy, w


# ---- environment maps (cfhip_equirect_to_cube_device, cfhip_cube_prefilter_device, cfhip_cube_sh9_device) ----
ENV_MAX_FACE = 8192
ENV_MAX_PANORAMA = 32768
ENV_SUPERSAMPLES = (1, 2, 4)
ENV_MIN_SAMPLES, ENV_MAX_SAMPLES = 64, 4096


class GgxSample(ctypes.Structure):
    """cfhip_ggx_sample: a tangent-space light direction (lz is also its weight) and a source level of detail"""
    _fields_ = [("lx", ctypes.c_float), ("ly", ctypes.c_float), ("lz", ctypes.c_float), ("lod", ctypes.c_float)]


class Sh9Result(ctypes.Structure):
    """cfhip_sh9_result: 9 coefficients x RGBA, normalised, then the sum of the texels' solid angles"""
    _fields_ = [("coeff", (ctypes.c_double*4)*9), ("solid_angle", ctypes.c_double)]


def cube_level_count(face_size: int) -> int:
    """the levels of a full chain: sizes face_size >> k down to 1"""
    return int(face_size).bit_length()


def _check_samples(samples) -> int:
    """the records of a sample table: a multiple of 64 from 64 to 4096"""
    if isinstance(samples, (bool, np.bool_)) or not isinstance(samples, (int, np.integer)) or samples % 64 \
            or not ENV_MIN_SAMPLES <= samples <= ENV_MAX_SAMPLES:
        raise ValueError("samples %r: a multiple of 64 from %d to %d" % (samples, ENV_MIN_SAMPLES, ENV_MAX_SAMPLES))
    return int(samples)


def ggx_sample_table(roughness: float, samples: int, face_size: int, source_levels: int) -> np.ndarray:
    """cfhip_ggx_sample_table -> (samples, 4) float32 records (lx, ly, lz, lod) for one destination level of
    cube_prefilter_device: `samples` Hammersley points (a multiple of 64 from 64 to 4096) through the GGX distribution
    of `roughness` (0 < roughness <= 1; 0 is a copy and has no table), the level of detail chosen per sample from its
    density for a source cube of face_size with source_levels levels.  Host only: no context, no device."""
    r = float(roughness)
    _check_samples(samples)
    if not (0.0 < r <= 1.0):
        raise ValueError("roughness %r outside (0, 1]: roughness 0 is a copy and has no table" % (roughness,))
    if not 1 <= int(face_size) <= ENV_MAX_FACE or not 1 <= int(source_levels) <= cube_level_count(face_size):
        raise ValueError("face_size %r with source_levels %r" % (face_size, source_levels))
    out = np.empty((int(samples), 4), np.float32)
    rc = load_library().cfhip_ggx_sample_table(r, int(samples), int(face_size), int(source_levels),
                                               out.ctypes.data_as(ctypes.POINTER(GgxSample)))
    if rc != 0:
        raise ValueError("cfhip_ggx_sample_table refused (%r, %r, %r, %r)" % (roughness, samples, face_size, source_levels))
    return out


# the real basis in the order 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2 (csrc/envmap.h)
SH_C0, SH_C1, SH_C2 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792
SH_C20, SH_C22 = 0.31539156525252005, 0.5462742152960396


def sh9_irradiance(coeffs, directions) -> np.ndarray:
    """The diffuse term from the nine coefficients of Context.cube_sh9: each band times its cosine-lobe factor (pi,
    2 pi / 3, pi / 4), evaluated at unit `directions` (..., 3) -> (..., C) for coeffs of shape (9, C)."""
    d = np.asarray(directions, np.float64)
    k = np.asarray(coeffs, np.float64)
    if k.ndim != 2 or k.shape[0] != 9 or d.shape[-1] != 3:
        raise ValueError("expected coeffs (9, C) and directions (..., 3)")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    basis = [SH_C0*np.ones_like(x), SH_C1*y, SH_C1*z, SH_C1*x, SH_C2*(x*y), SH_C2*(y*z), SH_C20*(3.0*(z*z) - 1.0),
             SH_C2*(x*z), SH_C22*(x*x - y*y)]
    band = [np.pi] + [2.0*np.pi/3.0]*3 + [np.pi/4.0]*5
    return sum((band[b]*basis[b])[..., None]*k[b] for b in range(9))


# ---- the other lobes, the BRDF lookup table, the irradiance cube (cfhip_lobe_sample_table, cfhip_hammersley_table,
# cfhip_brdf_lut_device, cfhip_cube_irradiance_device) ----
LOBE_GGX, LOBE_CHARLIE, LOBE_LAMBERT = 0, 1, 2      # enum CFHIP_LOBE_*
ENV_MAX_LUT = 1024


class HammersleySample(ctypes.Structure):
    """cfhip_hammersley_sample: cos and sin of phi = 2 pi xi2, then xi1, of one Hammersley point"""
    _fields_ = [("cos_phi", ctypes.c_float), ("sin_phi", ctypes.c_float), ("xi1", ctypes.c_float),
                ("reserved", ctypes.c_float)]


def lobe_sample_table(kind: int, roughness: float, samples: int, face_size: int, source_levels: int) -> np.ndarray:
    """cfhip_lobe_sample_table -> (samples, 4) float32 records (lx, ly, lz, lod) for one destination level of
    cube_prefilter_device, from the Hammersley points of ggx_sample_table.  kind LOBE_GGX: ggx_sample_table's records;
    LOBE_CHARLIE: the sheen distribution of `roughness` (0 < roughness <= 1); LOBE_LAMBERT: uniform over the hemisphere
    (roughness is not read) -- the prefilter weighs by lz, so the level is the irradiance over pi.  Host only."""
    if isinstance(kind, (bool, np.bool_)) or kind not in (LOBE_GGX, LOBE_CHARLIE, LOBE_LAMBERT):
        raise ValueError("kind %r: LOBE_GGX, LOBE_CHARLIE or LOBE_LAMBERT" % (kind,))
    r = 1.0 if kind == LOBE_LAMBERT else float(roughness)
    S = _check_samples(samples)
    if not (0.0 < r <= 1.0):
        raise ValueError("roughness %r outside (0, 1]: roughness 0 is a copy and has no table" % (roughness,))
    if not 1 <= int(face_size) <= ENV_MAX_FACE or not 1 <= int(source_levels) <= cube_level_count(face_size):
        raise ValueError("face_size %r with source_levels %r" % (face_size, source_levels))
    out = np.empty((S, 4), np.float32)
    rc = load_library().cfhip_lobe_sample_table(int(kind), r, S, int(face_size), int(source_levels),
                                                out.ctypes.data_as(ctypes.POINTER(GgxSample)))
    if rc != 0:
        raise ValueError("cfhip_lobe_sample_table refused (%r, %r, %r, %r, %r)" % (kind, roughness, samples, face_size,
                                                                                   source_levels))
    return out


def hammersley_table(samples: int) -> np.ndarray:
    """cfhip_hammersley_table -> (samples, 4) float32 records (cos phi, sin phi, xi1, 0) of the Hammersley points every
    sample table here is made from: what brdf_lut_device reads.  Host only: no context, no device."""
    S = _check_samples(samples)
    out = np.empty((S, 4), np.float32)
    if load_library().cfhip_hammersley_table(S, out.ctypes.data_as(ctypes.POINTER(HammersleySample))) != 0:
        raise ValueError("cfhip_hammersley_table refused %r" % (samples,))
    return out


RDO_NO_CAP = 0xFFFFFFFF         # max_sse_increase: no cap
RDO_ROW_ABOVE = 1               # CFHIP_RDO_ROW_ABOVE

DECODE_NATIVE = -1              # CFHIP_DECODE_NATIVE
# output texel (channels, dtype) of a batched decode to a pixel type
PIXEL_ARRAY = {PixelType.RGBA8: (4, np.uint8), PixelType.RGBA32F: (4, np.float32), PixelType.RGBA16F: (4, np.float16)}


class ImageOps(ctypes.Structure):
    """struct cfhip_image_ops"""
    _fields_ = [("ops", ctypes.c_uint32), ("src_color_space", ctypes.c_int32), ("dst_color_space", ctypes.c_int32),
                ("rotate", ctypes.c_int32), ("normal_options", ctypes.c_uint32), ("rgbf", ctypes.c_uint32),
                ("normal_height", ctypes.c_double), ("swizzle", ctypes.c_int32 * 4)]


def make_image_ops(ops=0, src_color_space=ColorSpace.Linear, dst_color_space=None, rotate=RotateAngle.CW90,
                   normal_options=NormalOptions.Default, normal_height=1.0,
                   swizzle=(Channel.Red, Channel.Green, Channel.Blue, Channel.Alpha), rgbf=False) -> ImageOps:
    """An ImageOps descriptor; dst_color_space None = the image's own."""
    o = ImageOps()
    o.ops = int(ops)
    o.src_color_space = int(src_color_space)
    o.dst_color_space = int(src_color_space if dst_color_space is None else dst_color_space)
    o.rotate = int(rotate)
    o.normal_options = int(normal_options)
    o.rgbf = 1 if rgbf else 0
    o.normal_height = float(normal_height)
    for i in range(4):
        o.swizzle[i] = int(swizzle[i])
    return o


class CfhipError(RuntimeError):
    def __init__(self, code: int, text: str, status: Optional[int] = None, bad_chunk: Optional[int] = None):
        super().__init__("cfhip error %d: %s" % (code, text))
        self.code = code
        self.status, self.bad_chunk = status, bad_chunk     # E_DATA: the error class and the lowest failing chunk
        self.bad_block = bad_chunk                          # ... which cfhip_lz4_decode calls a block


_lib = None


def load_library(path: Optional[str] = None):
    """dlopen libcuttlefish_hip.so.  torch (if importable) is imported first so the
    process holds ONE HIP runtime (torch bundles libamdhip64.so.7 with the same soname)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("CFHIP_LIB") or LIB_PATH   # CFHIP_LIB: A/B kernel variants
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the product has no CPU fallback)" % path)
    try:  # pragma: no cover - depends on environment
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    L.cfhip_abi_version.restype = ctypes.c_int
    L.cfhip_device_count.restype = ctypes.c_int
    L.cfhip_create.restype = ctypes.c_void_p
    L.cfhip_create.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_int)]
    L.cfhip_destroy.argtypes = [ctypes.c_void_p]
    L.cfhip_destroy.restype = None
    L.cfhip_query.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 3
    L.cfhip_query.restype = ctypes.c_int
    L.cfhip_encode.argtypes = [ctypes.c_void_p, ctypes.POINTER(Surface), ctypes.c_size_t,
                               ctypes.POINTER(Params)]
    L.cfhip_encode.restype = ctypes.c_int
    L.cfhip_encode_multi.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(Surface),
                                     ctypes.c_size_t, ctypes.POINTER(Params)]
    L.cfhip_encode_multi.restype = ctypes.c_int
    L.cfhip_encode_multi_ex.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(Surface),
                                        ctypes.c_size_t, ctypes.POINTER(Params), CONSUMED_FN, ctypes.c_void_p]
    L.cfhip_encode_multi_ex.restype = ctypes.c_int
    L.cfhip_encode_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(Surface), ctypes.c_size_t,
                                      ctypes.POINTER(Params), ctypes.c_void_p]
    L.cfhip_encode_device.restype = ctypes.c_int
    L.cfhip_shard_rows.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_uint32),
                                   ctypes.POINTER(ctypes.c_uint32)]
    L.cfhip_shard_rows.restype = ctypes.c_int
    L.cfhip_last_kernel_ms.argtypes = [ctypes.c_void_p]
    L.cfhip_last_kernel_ms.restype = ctypes.c_float
    L.cfhip_pinned_bytes.argtypes = [ctypes.c_void_p]
    L.cfhip_pinned_bytes.restype = ctypes.c_size_t
    L.cfhip_last_kernel_name.argtypes = [ctypes.c_void_p]
    L.cfhip_last_kernel_name.restype = ctypes.c_char_p
    L.cfhip_profile_begin.argtypes = [ctypes.c_void_p]
    L.cfhip_profile_begin.restype = ctypes.c_int
    L.cfhip_profile_end.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float),
                                    ctypes.POINTER(ctypes.c_uint32)]
    L.cfhip_profile_end.restype = ctypes.c_int
    L.cfhip_last_error.argtypes = [ctypes.c_void_p]
    L.cfhip_last_error.restype = ctypes.c_char_p
    L.cfhip_generate_mips_device.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
        ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
        ctypes.c_uint32, ctypes.c_void_p]
    L.cfhip_generate_mips_device.restype = ctypes.c_int
    L.cfhip_generate_mips_array_device.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
        ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
        ctypes.c_uint32, ctypes.c_void_p]
    L.cfhip_generate_mips_array_device.restype = ctypes.c_int
    L.cfhip_mip_post_array_device.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
        ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
        ctypes.POINTER(MipPostParams), ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_mip_post_array_device.restype = ctypes.c_int
    L.cfhip_alpha_coverage_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(CoverageSurface), ctypes.c_uint32,
                                              ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_alpha_coverage_device.restype = ctypes.c_int
    L.cfhip_alpha_bleed_array_device.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
        ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(BleedParams), ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_alpha_bleed_array_device.restype = ctypes.c_int
    L.cfhip_alpha_sdf_array_device.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
        ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_size_t,
        ctypes.POINTER(SdfParams), ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_alpha_sdf_array_device.restype = ctypes.c_int
    L.cfhip_spec_aa_array_device.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
        ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(SpecAaParams), ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_spec_aa_array_device.restype = ctypes.c_int
    L.cfhip_height_ao_array_device.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
        ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_size_t,
        ctypes.POINTER(HeightAoParams), ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_height_ao_array_device.restype = ctypes.c_int
    L.cfhip_height_ao_directions.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32),
                                             ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)]
    L.cfhip_height_ao_directions.restype = ctypes.c_int
    L.cfhip_equirect_to_cube_device.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.cfhip_equirect_to_cube_device.restype = ctypes.c_int
    L.cfhip_ggx_sample_table.argtypes = [ctypes.c_float, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.POINTER(GgxSample)]
    L.cfhip_ggx_sample_table.restype = ctypes.c_int
    L.cfhip_cube_prefilter_device.argtypes = [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_uint32,
        ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    L.cfhip_cube_prefilter_device.restype = ctypes.c_int
    L.cfhip_cube_sh9_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
                                        ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_cube_sh9_device.restype = ctypes.c_int
    L.cfhip_lobe_sample_table.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.POINTER(GgxSample)]
    L.cfhip_lobe_sample_table.restype = ctypes.c_int
    L.cfhip_hammersley_table.argtypes = [ctypes.c_uint32, ctypes.POINTER(HammersleySample)]
    L.cfhip_hammersley_table.restype = ctypes.c_int
    L.cfhip_brdf_lut_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.cfhip_brdf_lut_device.restype = ctypes.c_int
    L.cfhip_cube_irradiance_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                               ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.cfhip_cube_irradiance_device.restype = ctypes.c_int
    L.cfhip_generate_mips3d_device.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
        ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
        ctypes.c_uint32, ctypes.c_void_p]
    L.cfhip_generate_mips3d_device.restype = ctypes.c_int
    L.cfhip_resize_device.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t,
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.cfhip_resize_device.restype = ctypes.c_int
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.cfhip_decoded_layout.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                       ctypes.POINTER(ctypes.c_int)]
    L.cfhip_decoded_layout.restype = ctypes.c_int
    L.cfhip_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, u64p]
    L.cfhip_decode.restype = ctypes.c_int
    L.cfhip_decode_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                      ctypes.c_void_p]
    L.cfhip_decode_device.restype = ctypes.c_int
    L.cfhip_decode_sse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, u64p]
    L.cfhip_decode_sse.restype = ctypes.c_int
    L.cfhip_decode_sse_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_decode_sse_device.restype = ctypes.c_int
    L.cfhip_image_ops_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(ImageOps), ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_void_p]
    L.cfhip_image_ops_device.restype = ctypes.c_int
    u8p, fp = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_float)
    L.cfhip_compare.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, u8p,
                                ctypes.c_uint, ctypes.POINTER(CompareResult), fp, ctypes.c_size_t]
    L.cfhip_compare.restype = ctypes.c_int
    L.cfhip_compare_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, u8p,
                                       ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p]
    L.cfhip_compare_device.restype = ctypes.c_int
    L.cfhip_pvrtc_query.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.POINTER(ctypes.c_size_t)]
    L.cfhip_pvrtc_query.restype = ctypes.c_int
    for name in ("cfhip_pvrtc_encode", "cfhip_pvrtc_encode_device"):
        fn = getattr(L, name)
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(Surface), ctypes.c_size_t, ctypes.POINTER(Params)] + \
            ([ctypes.c_void_p] if name.endswith("device") else [])
        fn.restype = ctypes.c_int
    L.cfhip_pvrtc_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
    L.cfhip_pvrtc_decode.restype = ctypes.c_int
    L.cfhip_pvrtc_decode_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p]
    L.cfhip_pvrtc_decode_device.restype = ctypes.c_int
    L.cfhip_pvrtc_decode_sse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    L.cfhip_pvrtc_decode_sse.restype = ctypes.c_int
    L.cfhip_pvrtc_decode_sse_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_pvrtc_decode_sse_device.restype = ctypes.c_int
    L.cfhip_std_unpack.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
    L.cfhip_std_unpack.restype = ctypes.c_int
    L.cfhip_std_unpack_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p]
    L.cfhip_std_unpack_device.restype = ctypes.c_int
    L.cfhip_std_compare.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t,
                                    u8p, ctypes.c_uint, ctypes.POINTER(CompareResult)]
    L.cfhip_std_compare.restype = ctypes.c_int
    L.cfhip_std_compare_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_size_t, u8p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_std_compare_device.restype = ctypes.c_int
    L.cfhip_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(DecodeSurface), ctypes.c_size_t, u64p]
    L.cfhip_decode_batch.restype = ctypes.c_int
    L.cfhip_decode_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(DecodeSurface), ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_void_p]
    L.cfhip_decode_batch_device.restype = ctypes.c_int
    L.cfhip_compare_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(CompareSurface),
                                      ctypes.c_size_t, ctypes.c_int, u8p, ctypes.c_uint, ctypes.c_void_p]
    L.cfhip_compare_batch.restype = ctypes.c_int
    L.cfhip_compare_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(CompareSurface), ctypes.c_size_t, ctypes.c_int, u8p,
                                             ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_compare_batch_device.restype = ctypes.c_int
    L.cfhip_rdo_supported.argtypes = [ctypes.c_int, ctypes.c_int]
    L.cfhip_rdo_supported.restype = ctypes.c_int
    L.cfhip_rdo.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RdoSurface), ctypes.c_size_t,
                            ctypes.POINTER(RdoParams), u8p, ctypes.c_void_p]
    L.cfhip_rdo.restype = ctypes.c_int
    L.cfhip_rdo_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RdoSurface),
                                   ctypes.c_size_t, ctypes.POINTER(RdoParams), u8p, ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_rdo_device.restype = ctypes.c_int
    L.cfhip_rdo_ex.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RdoSurface), ctypes.c_size_t,
                               ctypes.POINTER(RdoExParams), u8p, ctypes.c_void_p]
    L.cfhip_rdo_ex.restype = ctypes.c_int
    L.cfhip_rdo_ex_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RdoSurface),
                                      ctypes.c_size_t, ctypes.POINTER(RdoExParams), u8p, ctypes.c_void_p,
                                      ctypes.c_void_p]
    L.cfhip_rdo_ex_device.restype = ctypes.c_int
    L.cfhip_lz_size.argtypes = [ctypes.c_void_p, ctypes.POINTER(LzSpan), ctypes.c_size_t, ctypes.c_void_p]
    L.cfhip_lz_size.restype = ctypes.c_int
    L.cfhip_lz_size_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(LzSpan), ctypes.c_size_t, ctypes.c_void_p,
                                       ctypes.c_void_p]
    L.cfhip_lz_size_device.restype = ctypes.c_int
    L.cfhip_lz_slice_bytes.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    L.cfhip_lz_slice_bytes.restype = ctypes.c_size_t
    L.cfhip_deflate_bound.argtypes = [ctypes.c_size_t]
    L.cfhip_deflate_bound.restype = ctypes.c_size_t
    L.cfhip_deflate.argtypes = [ctypes.c_void_p, ctypes.POINTER(LzSpan), ctypes.c_size_t, ctypes.c_void_p,
                                ctypes.c_size_t, ctypes.c_void_p]
    L.cfhip_deflate.restype = ctypes.c_int
    L.cfhip_deflate_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(LzSpan), ctypes.c_size_t, ctypes.c_void_p,
                                       ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_deflate_device.restype = ctypes.c_int
    L.cfhip_deflate_code_lengths.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                                             ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint8)]
    L.cfhip_deflate_code_lengths.restype = ctypes.c_int
    L.cfhip_zindex_entries.argtypes = [ctypes.c_size_t]
    L.cfhip_zindex_entries.restype = ctypes.c_size_t
    L.cfhip_deflate_indexed.argtypes = [ctypes.c_void_p, ctypes.POINTER(LzSpan), ctypes.c_size_t, ctypes.c_void_p,
                                        ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.cfhip_deflate_indexed.restype = ctypes.c_int
    L.cfhip_deflate_indexed_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(LzSpan), ctypes.c_size_t, ctypes.c_void_p,
                                               ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                               ctypes.c_void_p]
    L.cfhip_deflate_indexed_device.restype = ctypes.c_int
    L.cfhip_inflate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.cfhip_inflate.restype = ctypes.c_int
    L.cfhip_inflate_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_inflate_device.restype = ctypes.c_int
    L.cfhip_lz4_bound.argtypes = [ctypes.c_size_t]
    L.cfhip_lz4_bound.restype = ctypes.c_size_t
    L.cfhip_lz4_encode.argtypes = [ctypes.c_void_p, ctypes.POINTER(LzSpan), ctypes.c_size_t, ctypes.c_void_p,
                                   ctypes.c_size_t, ctypes.c_void_p]
    L.cfhip_lz4_encode.restype = ctypes.c_int
    L.cfhip_lz4_encode_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(LzSpan), ctypes.c_size_t, ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_lz4_encode_device.restype = ctypes.c_int
    L.cfhip_lz4_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.c_void_p]
    L.cfhip_lz4_decode.restype = ctypes.c_int
    L.cfhip_lz4_decode_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.cfhip_lz4_decode_device.restype = ctypes.c_int
    for name, takes_n in (("lz", False), ("deflate", False), ("inflate", False), ("lz4_encode", True), ("lz4_decode", True),
                          ("png", False)):
        f = getattr(L, "cfhip_%s_stage_ms" % name)
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)] + ([ctypes.c_size_t] if takes_n else [])
        f.restype = ctypes.c_int
    L.cfhip_png_bound.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.cfhip_png_bound.restype = ctypes.c_size_t
    L.cfhip_png_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32,
                                   ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                   ctypes.c_size_t, ctypes.c_void_p]
    L.cfhip_png_encode.restype = ctypes.c_int
    L.cfhip_png_encode_device.argtypes = L.cfhip_png_encode.argtypes + [ctypes.c_void_p]
    L.cfhip_png_encode_device.restype = ctypes.c_int
    L.cfhip_rdo_target.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RdoSurface),
                                   ctypes.c_size_t, ctypes.POINTER(RdoExParams), ctypes.POINTER(ctypes.c_uint8),
                                   ctypes.c_void_p, ctypes.c_float, ctypes.POINTER(RdoTargetResult)]
    L.cfhip_rdo_target.restype = ctypes.c_int
    L.cfhip_rdo_target_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RdoSurface),
                                          ctypes.c_size_t, ctypes.POINTER(RdoExParams), ctypes.POINTER(ctypes.c_uint8),
                                          ctypes.c_void_p, ctypes.c_float, ctypes.POINTER(RdoTargetResult),
                                          ctypes.c_void_p]
    L.cfhip_rdo_target_device.restype = ctypes.c_int
    L.cfhip_decode_out_supported.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.cfhip_decode_out_supported.restype = ctypes.c_int
    _lib = L
    return L


def make_params(fmt, typ=Type.UNorm, quality=Quality.Normal, alpha=Alpha.Standard,
                color_mask: Sequence[bool] = (True, True, True, True),
                color_space=ColorSpace.Linear) -> Params:
    p = Params()
    p.format, p.type, p.quality = int(fmt), int(typ), int(quality)
    p.alpha, p.color_space = int(alpha), int(color_space)
    for i in range(4):
        p.mask_rgba[i] = 1 if color_mask[i] else 0
    return p


def query(fmt, typ=Type.UNorm):
    """(block_w, block_h, block_bytes) = Texture::blockWidth/Height/Size; raises on the
    (format, type) pairs createConverter rejects (Converter.cpp:339-412)."""
    bw, bh, bs = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = load_library().cfhip_query(int(fmt), int(typ), bw, bh, bs)
    if rc != 0:
        raise CfhipError(rc, "illegal (format, type) = (%r, %r)" % (fmt, typ))
    return bw.value, bh.value, bs.value


def payload_size(fmt, typ, width: int, height: int) -> int:
    bw, bh, bs = query(fmt, typ)
    return ((width + bw - 1) // bw) * ((height + bh - 1) // bh) * bs


def pvrtc_payload_size(fmt, typ, width: int, height: int) -> int:
    """Payload bytes of a PVRTC1 4 bpp level: max(w/4, 2) * max(h/4, 2) * 8.  Raises for other formats and types
    (CFHIP_E_UNSUPPORTED) and for sizes that are not powers of two (CFHIP_E_INVALID)."""
    n = ctypes.c_size_t()
    rc = load_library().cfhip_pvrtc_query(int(fmt), int(typ), width, height, ctypes.byref(n))
    if rc != 0:
        raise CfhipError(rc, "no PVRTC1 payload for (format, type) = (%r, %r) at %dx%d" % (fmt, typ, width, height))
    return n.value


def decoded_layout(fmt, typ=Type.UNorm):
    """(Layout, bytes per texel) of what decoding a (format, type) payload returns; raises for the standard
    formats and the pairs query() rejects."""
    lay, tb = ctypes.c_int(), ctypes.c_int()
    rc = load_library().cfhip_decoded_layout(int(fmt), int(typ), lay, tb)
    if rc != 0:
        raise CfhipError(rc, "no decoded layout for (format, type) = (%r, %r)" % (fmt, typ))
    return Layout(lay.value), tb.value


def decode_out_supported(fmt, typ, out_pixel=None) -> bool:
    """Whether a batched decode of (fmt, typ) can store out_pixel (None: the native layout).  Needs no device."""
    return bool(load_library().cfhip_decode_out_supported(int(fmt), int(typ),
                                                          DECODE_NATIVE if out_pixel is None else int(out_pixel)))


def rdo_supported(fmt, typ=Type.UNorm) -> bool:
    """Whether Context.rdo optimises payloads of this (format, type) pair: BC1-5 and BC7, UNorm."""
    return bool(load_library().cfhip_rdo_supported(int(fmt), int(typ)))


def make_rdo_params(lam: float, max_sse_increase: Optional[int] = None) -> RdoParams:
    p = RdoParams()
    p.lam = float(lam)
    p.max_sse_increase = RDO_NO_CAP if max_sse_increase is None else int(max_sse_increase)
    return p


def make_rdo_ex_params(lam: float, max_sse_increase: Optional[int] = None, row_above: bool = False,
                       window_bytes: Optional[int] = None) -> RdoExParams:
    """cfhip_rdo_ex_params: row_above lets a block copy from the block row above; window_bytes is the compressor's
    window (None: deflate's 32768)."""
    p = RdoExParams()
    p.struct_size = ctypes.sizeof(RdoExParams)
    p.lam = float(lam)
    p.max_sse_increase = RDO_NO_CAP if max_sse_increase is None else int(max_sse_increase)
    p.flags = RDO_ROW_ABOVE if row_above else 0
    p.window_bytes = 0 if window_bytes is None else int(window_bytes)
    return p


def psnr_from_sse(sse, n_texels: int, channels: int = 3) -> float:
    """PSNR (dB, peak 255) of the first `channels` sums of a decode_sse result over n_texels texels."""
    total = sum(int(v) for v in list(sse)[:channels])
    if total == 0:
        return float("inf")
    return 10.0 * float(np.log10(255.0 * 255.0 * n_texels * channels / total))


def shard_rows(block_rows: int, rank: int, world: int):
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    rc = load_library().cfhip_shard_rows(block_rows, rank, world, a, b)
    if rc != 0:
        raise CfhipError(rc, "bad shard arguments")
    return a.value, b.value


def pixel_type_of(arr: np.ndarray) -> PixelType:
    if arr.dtype == np.uint8:
        return PixelType.RGBA8
    if arr.dtype == np.float32:
        return PixelType.RGBA32F
    if arr.dtype == np.float16:
        return PixelType.RGBA16F
    raise TypeError("pixel dtype %s not accepted at the boundary" % arr.dtype)


# ---- marshalling: what the methods below hand to ctypes ----
def _ptr(x):
    """an optional pointer argument: an address, or 0 / None for NULL"""
    return ctypes.c_void_p(int(x)) if x else None


def _stream(s):
    """a stream argument: the caller's hipStream_t as an int, or 0 for the context's own"""
    return ctypes.c_void_p(s) if s else None


def _ptr_array(ptrs, n_min=1):
    """a C array of the addresses in ptrs, n_min entries at the least (an empty list still passes a pointer)"""
    ptrs = [ctypes.c_void_p(int(p)) for p in ptrs]
    return (ctypes.c_void_p * max(len(ptrs), n_min))(*ptrs)


def _same_layers(srcs, levels, names):
    """srcs[l] and levels[l][k-1] of the array calls -> (layers, the levels listed per layer)"""
    if len(srcs) == 0 or len(levels) != len(srcs) or len({len(d) for d in levels}) != 1:
        raise ValueError("%s and %s must list the same layers, every layer the same levels" % names)
    return len(srcs), len(levels[0])


def _rgba_host(image) -> np.ndarray:
    """one image as the host conveniences take it: contiguous and (h, w, 4)"""
    host = np.ascontiguousarray(image)
    if host.ndim != 3 or host.shape[2] != 4:
        raise ValueError("expected (h, w, 4)")
    return host


class Context:
    """One encoder context = one GPU (one process per GPU in multi-GPU jobs)."""

    def __init__(self, device_id: int = 0):
        self._lib = load_library()
        err = ctypes.c_int(0)
        self._h = self._lib.cfhip_create(device_id, 0, ctypes.byref(err))
        if not self._h:
            raise CfhipError(err.value, self._lib.cfhip_last_error(None).decode())
        self.device_id = device_id

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cfhip_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise CfhipError(rc, self._lib.cfhip_last_error(self._h).decode())

    def _upload(self, host: np.ndarray):
        """the bytes of a contiguous host array as a uint8 tensor on this context's device"""
        import torch
        return torch.from_numpy(host.view(np.uint8)).to("cuda:%d" % self.device_id)

    def _rgba_device(self, image):
        """one (h, w, 4) image of the host conveniences -> (its contiguous array, its pixel type, its bytes on the device)"""
        host = _rgba_host(image)
        return host, pixel_type_of(host), self._upload(host)

    def encode(self, images: Iterable[np.ndarray], params: Params):
        """Host-buffer path (what HipConverter::process calls): list of (h, w, 4) arrays
        -> list of payload byte arrays."""
        surf, outs, keep = self._host_surfaces(images, params)
        self._check(self._lib.cfhip_encode(self._h, surf, len(outs), ctypes.byref(params)))
        return outs

    def _host_surfaces(self, images, params):
        images = [np.asarray(im) for im in images]
        surf = (Surface * len(images))()
        outs, keep = [], []
        for i, im in enumerate(images):
            if im.ndim != 3 or im.shape[2] != 4:
                raise ValueError("surface %d: expected (h, w, 4)" % i)
            if im.strides[2] != im.itemsize or im.strides[1] != 4 * im.itemsize:
                im = np.ascontiguousarray(im)
            keep.append(im)
            h, w = im.shape[:2]
            out = np.zeros(payload_size(params.format, params.type, w, h), np.uint8)
            outs.append(out)
            surf[i].pixels = im.ctypes.data
            surf[i].pixel_type = int(pixel_type_of(im))
            surf[i].width, surf[i].height = w, h
            surf[i].row_pitch_bytes = im.strides[0]
            surf[i].out = out.ctypes.data
            surf[i].out_capacity = out.nbytes
        return surf, outs, keep

    def encode_multi(self, others: Sequence["Context"], images: Iterable[np.ndarray], params: Params,
                     consumed=None):
        """cfhip_encode_multi: this context plus `others` (one per GPU of this process) share the
        surfaces of the call by block count; same payloads as encode().  consumed(index): called (possibly
        from the contexts' worker threads) once the library has finished reading surface `index`
        (cfhip_encode_multi_ex: the hook through which HipConverter releases each source image)."""
        ctxs = [self] + list(others)
        surf, outs, keep = self._host_surfaces(images, params)
        arr = (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])
        if consumed is not None:
            cb = CONSUMED_FN(lambda user, i: consumed(int(i)))
            rc = self._lib.cfhip_encode_multi_ex(arr, len(ctxs), surf, len(outs), ctypes.byref(params), cb, None)
        else:
            rc = self._lib.cfhip_encode_multi(arr, len(ctxs), surf, len(outs), ctypes.byref(params))
        if rc != 0:
            for c in ctxs:
                c._check(rc)
        return outs

    def encode_device(self, surfaces: Sequence[dict], params: Params, stream: int = 0):
        """Device-buffer path.  surfaces: dicts with pixels (device ptr int), pixel_type,
        width, height, row_pitch_bytes, out (device ptr int), out_capacity."""
        surf = (Surface * len(surfaces))()
        for i, s in enumerate(surfaces):
            surf[i].pixels = s["pixels"]
            surf[i].pixel_type = int(s["pixel_type"])
            surf[i].width, surf[i].height = s["width"], s["height"]
            surf[i].row_pitch_bytes = s["row_pitch_bytes"]
            surf[i].out = s["out"]
            surf[i].out_capacity = s["out_capacity"]
        self._check(self._lib.cfhip_encode_device(self._h, surf, len(surfaces),
                                                   ctypes.byref(params),
                                                   _stream(stream)))

    def encode_pvrtc(self, images: Iterable[np.ndarray], params: Params):
        """PVRTC1 4 bpp (params.format 59 / 60): list of (h, w, 4) arrays, both sides powers of two (rows may run
        bottom-up: a negative row stride is passed on as a negative pitch) -> list of payload byte arrays.  All
        surfaces of the call share every launch."""
        images = [np.asarray(im) for im in images]
        surf = (Surface * len(images))()
        outs, keep = [], []
        for i, im in enumerate(images):
            if im.ndim != 3 or im.shape[2] != 4:
                raise ValueError("surface %d: expected (h, w, 4)" % i)
            if im.strides[2] != im.itemsize or im.strides[1] != 4 * im.itemsize:
                im = np.ascontiguousarray(im)
            keep.append(im)
            h, w = im.shape[:2]
            out = np.zeros(pvrtc_payload_size(params.format, params.type, w, h), np.uint8)
            outs.append(out)
            surf[i].pixels = im.ctypes.data
            surf[i].pixel_type = int(pixel_type_of(im))
            surf[i].width, surf[i].height = w, h
            surf[i].row_pitch_bytes = im.strides[0]
            surf[i].out = out.ctypes.data
            surf[i].out_capacity = out.nbytes
        self._check(self._lib.cfhip_pvrtc_encode(self._h, surf, len(outs), ctypes.byref(params)))
        return outs

    def encode_pvrtc_device(self, surfaces: Sequence[dict], params: Params, stream: int = 0):
        """Device path of encode_pvrtc; surfaces: dicts as for encode_device."""
        surf = (Surface * len(surfaces))()
        for i, s in enumerate(surfaces):
            surf[i].pixels = s["pixels"]
            surf[i].pixel_type = int(s["pixel_type"])
            surf[i].width, surf[i].height = s["width"], s["height"]
            surf[i].row_pitch_bytes = s["row_pitch_bytes"]
            surf[i].out = s["out"]
            surf[i].out_capacity = s["out_capacity"]
        self._check(self._lib.cfhip_pvrtc_encode_device(self._h, surf, len(surfaces), ctypes.byref(params),
                                                         _stream(stream)))

    def decode_pvrtc(self, payload: np.ndarray, fmt, width: int, height: int, typ=Type.UNorm):
        """PVRTC1 4 bpp payload -> (height, width, 4) uint8 (alpha 255 for the RGB format)"""
        blocks = np.ascontiguousarray(payload, dtype=np.uint8)
        out = np.empty((height, width, 4), np.uint8)
        self._check(self._lib.cfhip_pvrtc_decode(self._h, int(fmt), int(typ), blocks.ctypes.data, blocks.nbytes,
                                                 width, height, out.ctypes.data, out.nbytes))
        return out

    def decode_pvrtc_device(self, blocks: int, fmt, width: int, height: int, out: int, out_pitch_bytes: int,
                            typ=Type.UNorm, stream: int = 0):
        """Device path of decode_pvrtc: blocks / out are device pointers as ints (4-byte aligned)."""
        self._check(self._lib.cfhip_pvrtc_decode_device(
            self._h, int(fmt), int(typ), ctypes.c_void_p(int(blocks)), width, height, ctypes.c_void_p(int(out)),
            out_pitch_bytes, _stream(stream)))

    def decode_pvrtc_sse(self, payload: np.ndarray, ref: np.ndarray, fmt, typ=Type.UNorm):
        """Per-channel sums of squared differences between the decoded PVRTC1 payload and an (h, w, 4) uint8
        reference (its size is the surface's)."""
        ref = np.asarray(ref)
        if ref.ndim != 3 or ref.shape[2] != 4 or ref.dtype != np.uint8:
            raise ValueError("reference must be (h, w, 4) uint8")
        if ref.strides[2] != 1 or ref.strides[1] != 4 or ref.strides[0] < 0:
            ref = np.ascontiguousarray(ref)
        h, w = ref.shape[:2]
        blocks = np.ascontiguousarray(payload, dtype=np.uint8)
        sse = (ctypes.c_uint64 * 4)()
        self._check(self._lib.cfhip_pvrtc_decode_sse(self._h, int(fmt), int(typ), blocks.ctypes.data, blocks.nbytes,
                                                     w, h, ref.ctypes.data, ref.strides[0], sse))
        return [int(v) for v in sse]

    def decode_pvrtc_sse_device(self, blocks: int, fmt, width: int, height: int, ref: int, ref_pitch_bytes: int,
                                sse: int, typ=Type.UNorm, stream: int = 0):
        """Device path of decode_pvrtc_sse: sse = device pointer to four uint64 (8-byte aligned, zeroed by the call)."""
        self._check(self._lib.cfhip_pvrtc_decode_sse_device(
            self._h, int(fmt), int(typ), ctypes.c_void_p(int(blocks)), width, height, ctypes.c_void_p(int(ref)),
            ref_pitch_bytes, ctypes.c_void_p(int(sse)), _stream(stream)))

    def generate_mips_device(self, src: int, pixel_type, width: int, height: int,
                             row_pitch_bytes: int, dst_levels: Sequence[int],
                             color_space=ColorSpace.Linear, filter=0, stream: int = 0):
        """Texture::generateMipmaps on the GPU: level k (k = 1..len(dst_levels)) of a width x height
        texture into dst_levels[k-1] (device pointers, RGBA32F tightly packed), each level resized
        from the previous one in linear space.  filter: ResizeFilter (0 Box, 1 Linear)."""
        self._check(self._lib.cfhip_generate_mips_device(
            self._h, ctypes.c_void_p(int(src)), int(pixel_type), width, height, row_pitch_bytes,
            int(color_space), int(filter), _ptr_array(dst_levels), len(dst_levels) + 1, _stream(stream)))

    def generate_mips_array_device(self, srcs: Sequence[int], pixel_type, width: int, height: int,
                                   row_pitch_bytes: int, dst_levels: Sequence[Sequence[int]],
                                   color_space=ColorSpace.Linear, filter=0, stream: int = 0):
        """generate_mips_device for the layers of an array / cube texture in one call: srcs[l] = level 0
        of layer l, dst_levels[l][k-1] receives its level k.  One launch per pass and level for all
        layers; bit-identical to one call per layer."""
        nl, per = _same_layers(srcs, dst_levels, ("srcs", "dst_levels"))
        self._check(self._lib.cfhip_generate_mips_array_device(
            self._h, _ptr_array(srcs), nl, int(pixel_type), width, height, row_pitch_bytes, int(color_space), int(filter),
            _ptr_array([p for d in dst_levels for p in d]), per + 1, _stream(stream)))

    def mip_post_device(self, srcs: Sequence[int], pixel_type, width: int, height: int, row_pitch_bytes: int,
                        levels: Sequence[Sequence[int]], alpha_coverage: Optional[float] = None,
                        normalize: Optional[str] = None, results: int = 0, stream: int = 0):
        """The repairs of generated mip chains in place (cfhip_mip_post_array_device), on the buffers as
        generate_mips_array_device takes them: srcs[l] = level 0 of layer l (only read), levels[l][k-1] = its level k
        (RGBA32F, tightly packed).  alpha_coverage = t scales each level's alpha so that its share of texels with
        alpha >= t matches level 0's; normalize = "unorm" / "snorm" renormalises every RGB.  results: device pointer to
        len(srcs) * len(levels[0]) cfhip_mip_post_result records (MIP_POST_RESULT_DTYPE), required with alpha_coverage.
        Premultiplied colour is out of scope: the pass scales alpha alone, so run it on straight alpha."""
        nl, per = _same_layers(srcs, levels, ("srcs", "levels"))
        params = make_mip_post_params(alpha_coverage, normalize)
        self._check(self._lib.cfhip_mip_post_array_device(
            self._h, _ptr_array(srcs), nl, int(pixel_type), width, height, row_pitch_bytes,
            _ptr_array([p for d in levels for p in d]), per + 1, ctypes.byref(params), _ptr(results), _stream(stream)))

    def alpha_coverage_device(self, surfaces: Sequence[dict], threshold: float, counts: int, scale: float = 1.0,
                              stream: int = 0):
        """counts[i] (device pointer to len(surfaces) uint32) = the texels of surface i with fl32(alpha * scale) >=
        threshold.  surfaces: dicts with pixels (device ptr int), pixel_type, width, height, row_pitch_bytes; any mix
        of sizes and pixel types, one launch."""
        surf = (CoverageSurface * max(len(surfaces), 1))()
        for i, s in enumerate(surfaces):
            surf[i].pixels = s["pixels"]
            surf[i].pixel_type = int(s["pixel_type"])
            surf[i].width, surf[i].height = s["width"], s["height"]
            surf[i].pitch_bytes = s["row_pitch_bytes"]
        self._check(self._lib.cfhip_alpha_coverage_device(
            self._h, surf, len(surfaces), threshold, scale, _ptr(counts),
            _stream(stream)))

    def alpha_coverage(self, image: np.ndarray, threshold: float, scale: float = 1.0) -> int:
        """Host convenience: the number of texels of an (h, w, 4) uint8 / float16 / float32 image whose alpha passes
        fl32(alpha * scale) >= threshold, counted on the GPU."""
        import torch
        host, pt, dev = self._rgba_device(image)
        out = torch.zeros(1, dtype=torch.int32, device=dev.device)
        self.alpha_coverage_device([dict(pixels=dev.data_ptr(), pixel_type=pt, width=host.shape[1], height=host.shape[0],
                                         row_pitch_bytes=host.strides[0])], threshold, out.data_ptr(), scale)
        return int(out.cpu().numpy().view(np.uint32)[0])

    def alpha_bleed_device(self, images: Sequence[int], pixel_type, width: int, height: int, row_pitch_bytes: int,
                           threshold: float = 0.0, wrap=(False, False), max_distance: int = 0, results: int = 0,
                           stream: int = 0):
        """Alpha bleeding in place (cfhip_alpha_bleed_array_device): on each of the device surfaces images[l] (all of
        one size and pixel type) every texel with alpha <= threshold takes the R, G, B bits of the nearest texel with
        alpha > threshold, found by a jump flood; alpha is untouched.  wrap: a bool or (x, y), the axes on which the
        surface tiles; max_distance: how far a colour may travel, 0 = unlimited.  results: device pointer to len(images)
        cfhip_bleed_result records (BLEED_RESULT_DTYPE), or 0 for none.  One call is 2 + log2(P) launches whatever the
        number of layers, and takes 8 bytes of the context's scratch per texel.  The remedy for straight alpha: run it
        before mips and encoding, not on premultiplied colour."""
        params = make_bleed_params(threshold, wrap, max_distance)
        self._check(self._lib.cfhip_alpha_bleed_array_device(
            self._h, _ptr_array(images), len(images), int(pixel_type), width, height, row_pitch_bytes, ctypes.byref(params),
            _ptr(results), _stream(stream)))

    def alpha_bleed(self, image: np.ndarray, threshold: float = 0.0, wrap=(False, False), max_distance: int = 0):
        """Host convenience: one (h, w, 4) uint8 / float16 / float32 image through alpha_bleed_device -> (the bled
        array of the same dtype, the record as a dict of seeds, filled, max_dist2, reserved)."""
        import torch
        host, pt, dev = self._rgba_device(image)
        res = torch.zeros(4, dtype=torch.int32, device=dev.device)
        self.alpha_bleed_device([dev.data_ptr()], pt, host.shape[1], host.shape[0], host.strides[0], threshold, wrap,
                                max_distance, res.data_ptr())
        rec = res.cpu().numpy().view(BLEED_RESULT_DTYPE)[0]
        return dev.cpu().numpy().view(host.dtype), {k: int(rec[k]) for k in rec.dtype.names}

    def alpha_sdf_device(self, srcs: Sequence[int], pixel_type, width: int, height: int, row_pitch_bytes: int,
                         dsts: Sequence[int], dst_pixel_type, dst_row_pitch_bytes: int, spread: int, scale: int = 1,
                         threshold: float = 0.5, wrap=(False, False), channels="a", results: int = 0, stream: int = 0):
        """A signed distance field from alpha (cfhip_alpha_sdf_array_device): the texels of each device surface srcs[l]
        (all of one size and pixel type) with alpha > threshold are inside; every texel's Euclidean distance to the
        nearest texel of the other class, exact up to `spread` source texels, is averaged over scale x scale tiles and
        written to the `channels` of dsts[l] (width/scale x height/scale texels of dst_pixel_type) with 0.5 at the
        silhouette, 0 a spread outside it and 1 a spread inside.  The other components of dsts[l] are not written;
        dsts[l] may be srcs[l] at scale 1 with equal pixel types.  wrap: a bool or (x, y), the axes on which the
        surface tiles.  results: device pointer to len(srcs) cfhip_sdf_result records (SDF_RESULT_DTYPE), or 0 for none.
        One call is 3 launches at scale 1 and 4 above, whatever the layers and the spread."""
        nl = len(srcs)
        if len(dsts) != nl:
            raise ValueError("srcs and dsts must list the same layers")
        params = make_sdf_params(spread, scale, threshold, wrap, channels)
        self._check(self._lib.cfhip_alpha_sdf_array_device(
            self._h, _ptr_array(srcs), nl, int(pixel_type), width, height, row_pitch_bytes, _ptr_array(dsts),
            int(dst_pixel_type), dst_row_pitch_bytes, ctypes.byref(params), _ptr(results), _stream(stream)))

    def alpha_sdf(self, image: np.ndarray, spread: int, scale: int = 1, threshold: float = 0.5, wrap=(False, False),
                  channels="a", out_dtype=None):
        """Host convenience: one (h, w, 4) uint8 / float16 / float32 image through alpha_sdf_device -> (a new
        (h/scale, w/scale, 4) array of out_dtype -- the image's by default -- with the field in `channels`, the record as
        a dict of inside, saturated, reserved0, reserved1).  The other channels are zero, except at scale 1 with the
        image's own dtype, where they are the image's."""
        import torch
        host = _rgba_host(image)
        make_sdf_params(spread, scale, threshold, wrap, channels)
        h, w = host.shape[:2]
        if h % scale or w % scale:
            raise ValueError("%dx%d is not a multiple of the scale %d" % (w, h, scale))
        out_dtype = host.dtype if out_dtype is None else np.dtype(out_dtype)
        pt = pixel_type_of(host)
        dpt = pixel_type_of(np.empty(0, out_dtype))
        dev = self._upload(host)
        if scale == 1 and out_dtype == host.dtype:
            out = dev.clone()
        else:
            out = torch.zeros((h//scale, (w//scale)*4*out_dtype.itemsize), dtype=torch.uint8, device=dev.device)
        res = torch.zeros(4, dtype=torch.int32, device=dev.device)
        self.alpha_sdf_device([dev.data_ptr()], pt, w, h, host.strides[0], [out.data_ptr()], dpt,
                              (w//scale)*4*out_dtype.itemsize, spread, scale, threshold, wrap, channels, res.data_ptr())
        rec = res.cpu().numpy().view(SDF_RESULT_DTYPE)[0]
        return (out.cpu().numpy().view(out_dtype).reshape(h//scale, w//scale, 4),
                {k: int(rec[k]) for k in rec.dtype.names})

    def height_ao_device(self, srcs: Sequence[int], pixel_type, width: int, height: int, pitch: int, dsts: Sequence[int],
                         dst_pixel_type, dst_pitch: int, *, radius: int, height_scale: float = 1.0, directions: int = 16,
                         channel="r", channels="r", strength: float = 1.0, bias: float = 0.0, uniform: bool = False,
                         falloff: bool = False, wrap=(False, False), results: int = 0, stream: int = 0):
        """Ambient occlusion from height maps (cfhip_height_ao_array_device): `channel` of each device surface srcs[l]
        (all of one size and pixel type) is a height field, height_scale texels per stored unit; for every texel the
        highest horizon within `radius` texels is found in `directions` directions, and the share of the sky the
        horizons leave open -- 1 on a flat surface -- is written to the `channels` of dsts[l] (the same size, of
        dst_pixel_type).  The other components of dsts[l] are not written; dsts[l] may be srcs[l] with equal pixel
        types, whatever the channels.  The remaining arguments are make_height_ao_params'.  results: device pointer to
        len(srcs) cfhip_height_ao_result records (HEIGHT_AO_RESULT_DTYPE), or 0 for none.  One call is 2 launches,
        whatever the layers, directions and radius."""
        nl = len(srcs)
        if len(dsts) != nl:
            raise ValueError("srcs and dsts must list the same layers")
        params = make_height_ao_params(radius, height_scale, directions, channel, channels, strength, bias, uniform,
                                       falloff, wrap)
        self._check(self._lib.cfhip_height_ao_array_device(
            self._h, _ptr_array(srcs), nl, int(pixel_type), width, height, pitch, _ptr_array(dsts), int(dst_pixel_type),
            dst_pitch, ctypes.byref(params), _ptr(results), _stream(stream)))

    def height_ao(self, image: np.ndarray, radius: int, height_scale: float = 1.0, directions: int = 16, channel="r",
                  channels="r", strength: float = 1.0, bias: float = 0.0, uniform: bool = False, falloff: bool = False,
                  wrap=(False, False), out_dtype=None):
        """Host convenience: one (h, w, 4) uint8 / float16 / float32 image through height_ao_device -> (a new (h, w, 4)
        array of out_dtype -- the image's by default -- with the occlusion in `channels`, the record as a dict of
        occluded, darkest, reserved0, reserved1).  The other channels are the image's with its own dtype, else zero."""
        import torch
        host, pt, dev = self._rgba_device(image)
        kw = dict(radius=radius, height_scale=height_scale, directions=directions, channel=channel, channels=channels,
                  strength=strength, bias=bias, uniform=uniform, falloff=falloff, wrap=wrap)
        h, w = host.shape[:2]
        out_dtype = host.dtype if out_dtype is None else np.dtype(out_dtype)
        dpt = pixel_type_of(np.empty(0, out_dtype))
        if out_dtype == host.dtype:
            out = dev.clone()
        else:
            out = torch.zeros((h, w*4*out_dtype.itemsize), dtype=torch.uint8, device=dev.device)
        res = torch.zeros(4, dtype=torch.int32, device=dev.device)
        # the context's stream does not wait for torch's: the copy and the fills above must have landed before the pass
        # writes into the same memory
        torch.cuda.current_stream(dev.device).synchronize()
        self.height_ao_device([dev.data_ptr()], pt, w, h, host.strides[0], [out.data_ptr()], dpt, w*4*out_dtype.itemsize,
                              results=res.data_ptr(), **kw)
        rec = res.cpu().numpy().view(HEIGHT_AO_RESULT_DTYPE)[0]
        return out.cpu().numpy().view(out_dtype).reshape(h, w, 4), {k: int(rec[k]) for k in rec.dtype.names}

    def specular_aa_device(self, normals: Sequence[int], pixel_type, width: int, height: int, pitch: int,
                           levels: Sequence[Sequence[int]], *, rough0: Optional[Sequence[int]] = None,
                           rough_pixel_type=None, rough_pitch: int = 0, channel, perceptual: bool = True,
                           signed_normals: bool = False, reconstruct_z: bool = False, base_roughness: float = 0.5,
                           variance_scale: float = 1.0, max_variance: float = 1.0, results: int = 0, stream: int = 0):
        """Specular anti-aliasing of generated roughness chains in place (cfhip_spec_aa_array_device), on the buffers
        as generate_mips_array_device takes them: normals[l] = level 0 of layer l's normal map (only read),
        levels[l][k-1] = level k of its roughness chain (RGBA32F, tightly packed).  `channel` of every listed level is
        overwritten with sqrt of (the mean alpha^2 of the level-0 texels under the texel + variance_scale * the
        variance of their normals, as 1/kappa of the vMF lobe, at most max_variance); with perceptual the stored values
        are perceptual roughness (alpha = r^2).  The value written replaces the mip filter's own value in that channel:
        it is the footprint mean of alpha^2 plus the variance, not a correction of the filter's result.  Level 0, the
        other channels and the normals are never written.  rough0[l] = level 0 of the roughness map (rough_pixel_type,
        rows rough_pitch apart; it may be the normals' surface), or None: base_roughness in every texel.  results:
        device pointer to len(normals) * len(levels[0]) cfhip_spec_aa_result records (SPEC_AA_RESULT_DTYPE), or 0.
        One call is ceil(len(levels[0]) / 5) launches, at most 3, whatever the layers."""
        nl, per = _same_layers(normals, levels, ("normals", "levels"))
        if rough0 is not None and (len(rough0) != nl or rough_pixel_type is None):
            raise ValueError("rough0 lists the layers of normals and comes with its rough_pixel_type")
        params = make_spec_aa_params(channel, perceptual, signed_normals, reconstruct_z, base_roughness, variance_scale,
                                     max_variance)
        self._check(self._lib.cfhip_spec_aa_array_device(
            self._h, _ptr_array(normals), nl, int(pixel_type), width, height, pitch,
            _ptr_array(rough0) if rough0 is not None else None, int(rough_pixel_type) if rough0 is not None else 0,
            rough_pitch if rough0 is not None else 0, _ptr_array([p for d in levels for p in d]), per + 1,
            ctypes.byref(params), _ptr(results), _stream(stream)))

    def specular_aa(self, normals: np.ndarray, roughness0, levels_count: int, channel="g", perceptual: bool = True,
                    signed_normals: bool = False, reconstruct_z: bool = False, variance_scale: float = 1.0,
                    max_variance: float = 1.0):
        """Host convenience: one (h, w, 4) uint8 / float16 / float32 normal map and either its (h, w, 4) level-0
        roughness map or a float (the roughness of every texel) through specular_aa_device -> (the channel's levels
        1 ... levels_count - 1 as float32 arrays of (max(1, h >> k), max(1, w >> k)), the records as a list of dicts).
        The values do not depend on any mip filter: they are the footprint mean of alpha^2 plus the variance."""
        import torch
        host = _rgba_host(normals)
        h, w = host.shape[:2]
        ch = spec_aa_channel(channel)
        device = "cuda:%d" % self.device_id
        dev = self._upload(host)
        kw = dict(channel=ch, perceptual=perceptual, signed_normals=signed_normals, reconstruct_z=reconstruct_z,
                  variance_scale=variance_scale, max_variance=max_variance)
        keep = None
        if isinstance(roughness0, np.ndarray):
            rh = np.ascontiguousarray(roughness0)
            if rh.shape != host.shape:
                raise ValueError("the roughness map has the shape of the normal map")
            keep = self._upload(rh)
            kw.update(rough0=[keep.data_ptr()], rough_pixel_type=pixel_type_of(rh), rough_pitch=rh.strides[0])
        else:
            kw.update(base_roughness=float(roughness0))
        per = int(levels_count) - 1
        if per < 1:
            raise ValueError("levels_count is at least 2")
        lv = [torch.zeros((max(1, h >> k), max(1, w >> k), 4), dtype=torch.float32, device=device) for k in range(1, per + 1)]
        res = torch.zeros(per*4, dtype=torch.int32, device=device)
        self.specular_aa_device([dev.data_ptr()], pixel_type_of(host), w, h, host.strides[0], [[t.data_ptr() for t in lv]],
                                results=res.data_ptr(), **kw)
        rec = res.cpu().numpy().view(SPEC_AA_RESULT_DTYPE)
        return ([t.cpu().numpy()[:, :, ch].copy() for t in lv],
                [{k: int(r[k]) for k in rec.dtype.names} for r in rec])

    def equirect_to_cube_device(self, src: int, pixel_type, width: int, height: int, row_pitch_bytes: int,
                                faces: Sequence[int], face_size: int, supersample: int = 2, stream: int = 0):
        """An equirectangular panorama onto the six faces of a cube (cfhip_equirect_to_cube_device): src is one
        width x height device surface of any pixel type, read without a colour-space change; faces are six device
        pointers in CubeFace order, each face_size^2 tightly packed RGBA32F.  Every texel averages supersample^2 (1, 2
        or 4 per axis) bilinear fetches, x wrapped and y clamped; the panorama's centre column looks along +Z, its top
        row along +Y.  One launch."""
        if len(faces) != 6:
            raise ValueError("faces must list the six faces in CubeFace order")
        self._check(self._lib.cfhip_equirect_to_cube_device(
            self._h, ctypes.c_void_p(int(src)), int(pixel_type), width, height, row_pitch_bytes, _ptr_array(faces),
            face_size, supersample, _stream(stream)))

    def equirect_to_cube(self, image: np.ndarray, face_size: int, supersample: int = 2) -> List[np.ndarray]:
        """Host convenience: one (h, w, 4) uint8 / float16 / float32 panorama through equirect_to_cube_device -> the six
        (face_size, face_size, 4) float32 faces in CubeFace order."""
        import torch
        host = _rgba_host(image)
        if supersample not in ENV_SUPERSAMPLES:
            raise ValueError("supersample %r: one of %r" % (supersample, ENV_SUPERSAMPLES))
        if not 1 <= int(face_size) <= ENV_MAX_FACE:
            raise ValueError("face_size %r outside 1 to %d" % (face_size, ENV_MAX_FACE))
        n = int(face_size)
        dev = self._upload(host)
        out = torch.empty((6, n, n, 4), dtype=torch.float32, device=dev.device)
        self.equirect_to_cube_device(dev.data_ptr(), pixel_type_of(host), host.shape[1], host.shape[0], host.strides[0],
                                     [out[f].data_ptr() for f in range(6)], n, int(supersample))
        faces = out.cpu().numpy()
        return [faces[f] for f in range(6)]

    def cube_prefilter_device(self, src_levels: Sequence[Sequence[int]], face_size: int,
                              dst_levels: Sequence[Sequence[int]], tables: Sequence, stream: int = 0):
        """The GGX-prefiltered chain of a cube (cfhip_cube_prefilter_device).  src_levels[f][l]: device pointers of the
        cube's RGBA32F chain as generate_mips_array_device with the Box filter leaves it, level l of size
        max(1, face_size >> l); dst_levels[f][k]: where destination level k of that size goes.  tables[k]: the
        (S, 4) float32 records of ggx_sample_table for level k -- S a multiple of 64 from 64 to 4096 -- or None for a
        copy of source level k (roughness 0).  One launch per destination level for the six faces."""
        if len(src_levels) != 6 or len(dst_levels) != 6 or len({len(s) for s in src_levels}) != 1 \
                or len({len(d) for d in dst_levels}) != 1:
            raise ValueError("src_levels and dst_levels list six faces, every face the same levels")
        L, K = len(src_levels[0]), len(dst_levels[0])
        if len(tables) != K:
            raise ValueError("one table (or None) per destination level")
        keep = [None if t is None or len(t) == 0 else np.ascontiguousarray(t, dtype=np.float32) for t in tables]
        for t in keep:
            if t is not None and (t.ndim != 2 or t.shape[1] != 4):
                raise ValueError("a table is (S, 4) float32: lx, ly, lz, lod")
        tarr = _ptr_array([0 if t is None else t.ctypes.data for t in keep])
        counts = (ctypes.c_uint32 * max(K, 1))(*[0 if t is None else t.shape[0] for t in keep])
        self._check(self._lib.cfhip_cube_prefilter_device(
            self._h, _ptr_array([p for s in src_levels for p in s]), face_size, L,
            _ptr_array([p for d in dst_levels for p in d]), K, tarr, counts, _stream(stream)))

    def cube_prefilter(self, faces: Sequence[np.ndarray], roughness: Sequence[float], samples: int = 256):
        """Host convenience: six (n, n, 4) float32 faces in CubeFace order -> one (6, n_k, n_k, 4) float32 array per entry
        of `roughness`, n_k = max(1, n >> k): the full Box chain of the faces is built on the device, then level k is the
        environment under a GGX lobe of roughness[k] from `samples` samples; a roughness of 0 copies the Box level."""
        return self._cube_prefilter_tables(faces, len(roughness), lambda n, L: [
            None if float(r) == 0.0 else ggx_sample_table(r, samples, n, L) for r in roughness])

    def _cube_prefilter_tables(self, faces, K: int, make_tables):
        """what cube_prefilter and cube_prefilter_lobe share: the Box chain of the faces on the device, then K levels from
        make_tables(face size, source levels)"""
        import torch
        stack = np.ascontiguousarray(np.stack([np.asarray(f) for f in faces]), dtype=np.float32)
        if stack.ndim != 4 or stack.shape[0] != 6 or stack.shape[1] != stack.shape[2] or stack.shape[3] != 4:
            raise ValueError("expected six (n, n, 4) faces")
        n = stack.shape[1]
        L = cube_level_count(n)
        if not 1 <= K <= L:
            raise ValueError("%d levels asked of a face of %d: 1 to %d" % (K, n, L))
        tables = make_tables(n, L)
        device = "cuda:%d" % self.device_id
        chain = [torch.from_numpy(stack).to(device)]
        chain += [torch.empty((6, max(1, n >> l), max(1, n >> l), 4), dtype=torch.float32, device=device) for l in range(1, L)]
        if L > 1:
            self.generate_mips_array_device([chain[0][f].data_ptr() for f in range(6)], PixelType.RGBA32F, n, n, n*16,
                                            [[chain[l][f].data_ptr() for l in range(1, L)] for f in range(6)],
                                            color_space=ColorSpace.Linear, filter=int(ResizeFilter.Box))
        out = [torch.empty_like(chain[k]) for k in range(K)]
        self.cube_prefilter_device([[chain[l][f].data_ptr() for l in range(L)] for f in range(6)], n,
                                   [[out[k][f].data_ptr() for k in range(K)] for f in range(6)], tables)
        return [o.cpu().numpy() for o in out]

    def cube_sh9_device(self, faces: Sequence[int], face_size: int, result: int, stream: int = 0):
        """The projection of a cube on nine spherical-harmonic coefficients (cfhip_cube_sh9_device): faces are six
        device pointers in CubeFace order, each face_size^2 tightly packed RGBA32F; result: device pointer to one
        cfhip_sh9_result, 37 float64 -- coefficient b, channel c at [4 b + c], normalised by 4 pi over the summed
        solid angle, then that sum.  Two launches; identical calls give identical bytes."""
        if len(faces) != 6:
            raise ValueError("faces must list the six faces in CubeFace order")
        self._check(self._lib.cfhip_cube_sh9_device(self._h, _ptr_array(faces), face_size, _ptr(result), _stream(stream)))

    def cube_sh9(self, faces: Sequence[np.ndarray]):
        """Host convenience: six (n, n, 4) float32 faces -> (the (9, 4) float64 coefficients in the order 1, y, z, x, xy,
        yz, 3z^2 - 1, xz, x^2 - y^2, the summed solid angle).  sh9_irradiance() evaluates the diffuse term from them."""
        import torch
        stack = np.ascontiguousarray(np.stack([np.asarray(f) for f in faces]), dtype=np.float32)
        if stack.ndim != 4 or stack.shape[0] != 6 or stack.shape[1] != stack.shape[2] or stack.shape[3] != 4:
            raise ValueError("expected six (n, n, 4) faces")
        n = stack.shape[1]
        dev = torch.from_numpy(stack).to("cuda:%d" % self.device_id)
        res = torch.zeros(37, dtype=torch.float64, device=dev.device)
        self.cube_sh9_device([dev[f].data_ptr() for f in range(6)], n, res.data_ptr())
        rec = res.cpu().numpy()
        return rec[:36].reshape(9, 4).copy(), float(rec[36])

    def cube_prefilter_lobe(self, faces: Sequence[np.ndarray], kind: int, roughness: Sequence, samples: int = 256):
        """cube_prefilter with the tables of another lobe (lobe_sample_table): level k is the environment under the
        lobe `kind` of roughness[k].  An entry of None copies the Box level, as a roughness of 0 does for LOBE_GGX and
        LOBE_CHARLIE; LOBE_LAMBERT reads no roughness, so any other entry there is the uniform table.  The sheen
        distribution peaks at grazing half vectors, whose reflections point below the horizon: of a Charlie table only
        the share 2^-((2 a + 1) / (2 a)), a = roughness^2, carries weight (a third at roughness 1, one record in 512 at
        0.25), and a level no record is left for is a ValueError, not a face of NaN."""
        def make_tables(n, L):
            tables = [None if r is None or (kind != LOBE_LAMBERT and float(r) == 0.0)
                      else lobe_sample_table(kind, r, samples, n, L) for r in roughness]
            for r, t in zip(roughness, tables):
                if t is not None and not t[:, 2].any():
                    raise ValueError("roughness %r leaves none of %d samples above the horizon: more samples, or a rougher "
                                     "level" % (r, samples))
            return tables
        return self._cube_prefilter_tables(faces, len(roughness), make_tables)

    def brdf_lut_device(self, dst: int, width: int, height: int, table: np.ndarray, sheen: bool = False, stream: int = 0):
        """The BRDF lookup table of the split sum (cfhip_brdf_lut_device): dst is a device pointer to width x height (1
        to 1024 each) tightly packed RGBA32F; texel (x, y) holds, for N.V = (x + 0.5) / width and roughness
        (y + 0.5) / height, R and G = the scale and bias of F0 under GGX with the height-correlated Smith term, B = the
        Charlie sheen lobe's directional albedo when `sheen` (else 0), A = 1.  table: the (S, 4) float32 records of
        hammersley_table, S a multiple of 64 from 64 to 4096.  One launch; identical calls give identical bytes."""
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != 4:
            raise ValueError("the table is (S, 4) float32: cos phi, sin phi, xi1, 0")
        self._check(self._lib.cfhip_brdf_lut_device(self._h, _ptr(dst), width, height, ctypes.c_void_p(t.ctypes.data),
                                                    t.shape[0], int(bool(sheen)), _stream(stream)))

    def brdf_lut(self, width: int, height: int, samples: int = 1024, sheen: bool = False) -> np.ndarray:
        """Host convenience: brdf_lut_device with hammersley_table(samples) -> the (height, width, 4) float32 table."""
        import torch
        w, h = int(width), int(height)
        if not (1 <= w <= ENV_MAX_LUT and 1 <= h <= ENV_MAX_LUT):
            raise ValueError("width and height %r x %r outside 1 to %d" % (width, height, ENV_MAX_LUT))
        table = hammersley_table(samples)
        out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:%d" % self.device_id)
        self.brdf_lut_device(out.data_ptr(), w, h, table, sheen)
        return out.cpu().numpy()

    def cube_irradiance_device(self, sh9_result: int, faces: Sequence[int], face_size: int, over_pi: bool = False,
                               stream: int = 0):
        """The diffuse term as a cube (cfhip_cube_irradiance_device): sh9_result is the device pointer cube_sh9_device
        wrote its record to -- no host round trip -- and faces are six device pointers in CubeFace order, each
        face_size^2 tightly packed RGBA32F.  Every texel is sh9_irradiance at its direction, over pi with over_pi (what
        a shader multiplies by the albedo).  One launch."""
        if len(faces) != 6:
            raise ValueError("faces must list the six faces in CubeFace order")
        self._check(self._lib.cfhip_cube_irradiance_device(self._h, _ptr(sh9_result), _ptr_array(faces), face_size,
                                                           int(bool(over_pi)), _stream(stream)))

    def cube_irradiance(self, coeffs, face_size: int, over_pi: bool = False) -> np.ndarray:
        """Host convenience: the (9, C) coefficients of cube_sh9 (C up to 4; missing channels are 0) through
        cube_irradiance_device -> the (6, face_size, face_size, 4) float32 faces."""
        import torch
        k = np.asarray(coeffs, np.float64)
        if k.ndim != 2 or k.shape[0] != 9 or not 1 <= k.shape[1] <= 4:
            raise ValueError("expected coeffs (9, C), C from 1 to 4")
        if not 1 <= int(face_size) <= ENV_MAX_FACE:
            raise ValueError("face_size %r outside 1 to %d" % (face_size, ENV_MAX_FACE))
        n = int(face_size)
        rec = np.zeros(37, np.float64)
        rec[:36].reshape(9, 4)[:, :k.shape[1]] = k
        device = "cuda:%d" % self.device_id
        res = torch.from_numpy(rec).to(device)
        out = torch.empty((6, n, n, 4), dtype=torch.float32, device=device)
        self.cube_irradiance_device(res.data_ptr(), [out[f].data_ptr() for f in range(6)], n, over_pi)
        return out.cpu().numpy()

    def generate_mips3d_device(self, src: int, pixel_type, width: int, height: int, depth: int,
                               row_pitch_bytes: int, slice_pitch_bytes: int, dst_levels: Sequence[int],
                               color_space=ColorSpace.Linear, filter=0, stream: int = 0):
        """Texture::generateMipmaps for a 3-D texture on the GPU: level k into dst_levels[k-1] as
        max(1, depth >> k) tightly packed RGBA32F slices."""
        self._check(self._lib.cfhip_generate_mips3d_device(
            self._h, ctypes.c_void_p(int(src)), int(pixel_type), width, height, depth, row_pitch_bytes,
            slice_pitch_bytes, int(color_space), int(filter), _ptr_array(dst_levels), len(dst_levels) + 1, _stream(stream)))

    def resize_device(self, src: int, pixel_type, width: int, height: int, row_pitch_bytes: int,
                      dst: int, dst_width: int, dst_height: int, color_space=ColorSpace.Linear,
                      filter=0, stream: int = 0):
        """Image::resize on the GPU: src (device pointer) -> dst (device pointer, dst_width x
        dst_height RGBA32F tightly packed), in linear space."""
        self._check(self._lib.cfhip_resize_device(
            self._h, ctypes.c_void_p(int(src)), int(pixel_type), width, height, row_pitch_bytes,
            int(color_space), int(filter), ctypes.c_void_p(int(dst)), dst_width, dst_height,
            _stream(stream)))

    def image_ops_device(self, src: int, pixel_type, width: int, height: int, row_pitch_bytes: int, ops: ImageOps,
                         dst: int, dst_pitch_bytes: int, stream: int = 0):
        """Image's pixel ops in one pass on device buffers (cfhip_image_ops_device): src (width x height texels of
        pixel_type) -> dst (RGBA32F, height x width under a 90 / 270 degree rotation).  stream 0 = the context's
        stream (the call then synchronises)."""
        self._check(self._lib.cfhip_image_ops_device(
            self._h, _ptr(src), int(pixel_type), width, height, row_pitch_bytes,
            ctypes.byref(ops) if ops is not None else None, _ptr(dst),
            dst_pitch_bytes, _stream(stream)))

    def decode(self, payload: np.ndarray, fmt, typ, width: int, height: int):
        """Decode a payload on the GPU -> ((height, width, C) array in the layout's dtype, error blocks).
        RGBA16F layouts come back as float16 (the bit patterns the decoder produced)."""
        layout, tb = decoded_layout(fmt, typ)
        ch, dt = LAYOUT_ARRAY[layout]
        blocks = np.ascontiguousarray(payload, dtype=np.uint8)
        out = np.empty((height, width, ch), dt)
        bad = ctypes.c_uint64(0)
        self._check(self._lib.cfhip_decode(self._h, int(fmt), int(typ), blocks.ctypes.data, blocks.nbytes, width,
                                           height, out.ctypes.data, out.nbytes, ctypes.byref(bad)))
        return out, int(bad.value)

    def decode_device(self, blocks: int, fmt, typ, width: int, height: int, out: int, out_pitch_bytes: int,
                      error_blocks: int = 0, stream: int = 0):
        """Device path: blocks / out / error_blocks (one uint64, zeroed by the call; 0 = not counted) are device
        pointers as ints.  stream 0 = the context's stream (the call then synchronises)."""
        self._check(self._lib.cfhip_decode_device(
            self._h, int(fmt), int(typ), ctypes.c_void_p(int(blocks)), width, height, ctypes.c_void_p(int(out)),
            out_pitch_bytes, _ptr(error_blocks),
            _stream(stream)))

    def decode_batch(self, payloads: Sequence[np.ndarray], fmt, typ, sizes: Sequence, out_pixel=None):
        """Decode every surface of a call in one launch (cfhip_decode_batch).  payloads[i] is the payload of a
        sizes[i] = (width, height) surface.  out_pixel None: the native layout, arrays as decode() returns them;
        a PixelType: (h, w, 4) arrays of that type (decode_out_supported says which exist).  Payloads that lie
        one after the other in memory (Texture.load keeps them so) travel as one upload, the texels as one download.  -> (list of arrays, list of error-block counts)."""
        n = len(payloads)
        if len(sizes) != n:
            raise ValueError("payloads and sizes must list the same surfaces")
        if out_pixel is None:
            ch, dt = LAYOUT_ARRAY[decoded_layout(fmt, typ)[0]]
        else:
            ch, dt = PIXEL_ARRAY[PixelType(out_pixel)]
        tb = ch*np.dtype(dt).itemsize
        parts = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in payloads]
        total = sum(int(w)*int(h)*tb for w, h in sizes)
        texels = np.empty(max(total, 1), np.uint8)
        surf = (DecodeSurface*max(n, 1))()
        outs, to = [], 0
        for i, ((w, h), p) in enumerate(zip(sizes, parts)):
            w, h = int(w), int(h)
            surf[i].blocks, surf[i].blocks_bytes = p.ctypes.data, p.nbytes
            surf[i].width, surf[i].height = w, h
            surf[i].out, surf[i].out_pitch_bytes, surf[i].out_capacity = texels.ctypes.data + to, w*tb, w*h*tb
            outs.append(texels[to:to + w*h*tb].view(dt).reshape(h, w, ch))
            to += w*h*tb
        bad = (ctypes.c_uint64*max(n, 1))()
        self._check(self._lib.cfhip_decode_batch(self._h, int(fmt), int(typ),
                                                 DECODE_NATIVE if out_pixel is None else int(out_pixel), surf, n, bad))
        return outs, [int(bad[i]) for i in range(n)]

    def decode_batch_device(self, surfaces: Sequence[dict], fmt, typ, out_pixel=None, error_blocks: int = 0,
                            stream: int = 0):
        """Device path of decode_batch.  surfaces: dicts with blocks, out (device pointers as ints), width, height,
        out_pitch_bytes.  error_blocks: device pointer to len(surfaces) uint64 (zeroed by the call; 0 = not
        counted).  stream 0 = the context's stream (the call then synchronises)."""
        n = len(surfaces)
        surf = (DecodeSurface*max(n, 1))()
        for i, s in enumerate(surfaces):
            surf[i].blocks, surf[i].out = int(s["blocks"]), int(s["out"])
            surf[i].width, surf[i].height = s["width"], s["height"]
            surf[i].out_pitch_bytes = s["out_pitch_bytes"]
        self._check(self._lib.cfhip_decode_batch_device(
            self._h, int(fmt), int(typ), DECODE_NATIVE if out_pixel is None else int(out_pixel), surf, n,
            _ptr(error_blocks), _stream(stream)))

    def decode_sse(self, payload: np.ndarray, ref: np.ndarray, fmt, typ=Type.UNorm):
        """Per-channel sums of squared differences between the decoded payload and an (h, w, 4) uint8
        reference (its size is the surface's); 4 ints, 0 for channels the layout lacks."""
        ref = np.asarray(ref)
        if ref.ndim != 3 or ref.shape[2] != 4 or ref.dtype != np.uint8:
            raise ValueError("reference must be (h, w, 4) uint8")
        if ref.strides[2] != 1 or ref.strides[1] != 4:
            ref = np.ascontiguousarray(ref)
        h, w = ref.shape[:2]
        blocks = np.ascontiguousarray(payload, dtype=np.uint8)
        sse = (ctypes.c_uint64 * 4)()
        self._check(self._lib.cfhip_decode_sse(self._h, int(fmt), int(typ), blocks.ctypes.data, blocks.nbytes, w, h,
                                               ref.ctypes.data, ref.strides[0], sse))
        return [int(v) for v in sse]

    def decode_sse_device(self, blocks: int, fmt, typ, width: int, height: int, ref: int, ref_pitch_bytes: int,
                          sse: int, stream: int = 0):
        """Device path of decode_sse: sse = device pointer to four uint64 (8-byte aligned, zeroed by the call)."""
        self._check(self._lib.cfhip_decode_sse_device(
            self._h, int(fmt), int(typ), ctypes.c_void_p(int(blocks)), width, height, ctypes.c_void_p(int(ref)),
            ref_pitch_bytes, ctypes.c_void_p(int(sse)), _stream(stream)))

    @staticmethod
    def _mask(mask):
        if mask is None:
            return None
        m = list(mask)
        if len(m) != 4:
            raise ValueError("mask must have 4 entries (r, g, b, a)")
        return (ctypes.c_uint8 * 4)(*[1 if v else 0 for v in m])

    def compare(self, payload: np.ndarray, ref: np.ndarray, fmt, typ=Type.UNorm, mask=None, ssim: bool = False,
                block_map: bool = False) -> Comparison:
        """Decode a payload on the GPU and measure it against an (h, w, 4) uint8, float16 or float32 reference
        (its size is the surface's): SSE, log SSE (HDR layouts), reference maxima, SSIM (ssim=True, LDR layouts)
        and the per-block error map (block_map=True).  mask: 4 booleans (r, g, b, a), None = all."""
        ref = np.asarray(ref)
        pix = {np.dtype(np.uint8): PixelType.RGBA8, np.dtype(np.float32): PixelType.RGBA32F,
               np.dtype(np.float16): PixelType.RGBA16F}.get(ref.dtype)
        if ref.ndim != 3 or ref.shape[2] != 4 or pix is None:
            raise ValueError("reference must be (h, w, 4) uint8, float16 or float32")
        ref = np.ascontiguousarray(ref)
        h, w = ref.shape[:2]
        layout, _ = decoded_layout(fmt, typ)
        blocks = np.ascontiguousarray(payload, dtype=np.uint8)
        res = CompareResult()
        emap = None
        if block_map:
            bw, bh, _ = query(fmt, typ)
            emap = np.zeros(((h + bh - 1) // bh, (w + bw - 1) // bw), np.float32)
        self._check(self._lib.cfhip_compare(
            self._h, int(fmt), int(typ), blocks.ctypes.data, blocks.nbytes, w, h, ref.ctypes.data, int(pix),
            ref.strides[0], self._mask(mask), COMPARE_SSIM if ssim else 0, ctypes.byref(res),
            emap.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if emap is not None else None,
            emap.size if emap is not None else 0))
        return Comparison(res, layout, emap)

    def compare_device(self, blocks: int, fmt, typ, width: int, height: int, ref: int, ref_pixel_type,
                       ref_pitch_bytes: int, result: int, mask=None, ssim: bool = False, block_errors: int = 0,
                       block_errors_capacity: int = 0, stream: int = 0):
        """Device path of compare: blocks / ref / result (one cfhip_compare_result) / block_errors (floats, 0 =
        none) are device pointers as ints.  stream 0 = the context's stream (the call then synchronises)."""
        self._check(self._lib.cfhip_compare_device(
            self._h, int(fmt), int(typ), ctypes.c_void_p(int(blocks)), width, height, ctypes.c_void_p(int(ref)),
            int(ref_pixel_type), ref_pitch_bytes, self._mask(mask), COMPARE_SSIM if ssim else 0,
            ctypes.c_void_p(int(result)), _ptr(block_errors),
            block_errors_capacity, _stream(stream)))

    def compare_batch(self, payloads: Sequence[np.ndarray], refs: Sequence[np.ndarray], fmt, typ=Type.UNorm,
                      mask=None, ssim: bool = False, block_map: bool = False) -> List[Comparison]:
        """compare() for every surface of a call at once (cfhip_compare_batch): payloads[i] against refs[i], an
        (h, w, 4) array whose size is the surface's.  All refs must share one dtype (uint8, float16 or float32).
        The launch count does not depend on the number of surfaces, and each Comparison holds the bits compare()
        returns for its surface alone.  Payloads (and references) that lie one after the other in memory travel
        as one upload."""
        n = len(payloads)
        if len(refs) != n:
            raise ValueError("payloads and refs must list the same surfaces")
        layout, _ = decoded_layout(fmt, typ)
        if n == 0:
            return []
        refs = [np.asarray(r) for r in refs]
        if len({r.dtype for r in refs}) != 1:
            raise ValueError("all references of one compare_batch call must share one dtype")
        pix = {np.dtype(np.uint8): PixelType.RGBA8, np.dtype(np.float32): PixelType.RGBA32F,
               np.dtype(np.float16): PixelType.RGBA16F}.get(refs[0].dtype)
        if pix is None or any(r.ndim != 3 or r.shape[2] != 4 for r in refs):
            raise ValueError("references must be (h, w, 4) uint8, float16 or float32")
        refs = [np.ascontiguousarray(r) for r in refs]
        parts = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in payloads]
        surf = (CompareSurface*n)()
        maps = []
        if block_map:
            bw, bh, _ = query(fmt, typ)
        for i, (p, r) in enumerate(zip(parts, refs)):
            h, w = r.shape[:2]
            surf[i].blocks, surf[i].blocks_bytes = p.ctypes.data, p.nbytes
            surf[i].width, surf[i].height = w, h
            surf[i].ref, surf[i].ref_pitch_bytes = r.ctypes.data, r.strides[0]
            if block_map:
                maps.append(np.zeros(((h + bh - 1) // bh, (w + bw - 1) // bw), np.float32))
                surf[i].block_errors, surf[i].block_errors_capacity = maps[i].ctypes.data, maps[i].size
        res = (CompareResult*n)()
        self._check(self._lib.cfhip_compare_batch(self._h, int(fmt), int(typ), surf, n, int(pix), self._mask(mask),
                                                  COMPARE_SSIM if ssim else 0, ctypes.addressof(res)))
        return [Comparison(res[i], layout, maps[i] if block_map else None) for i in range(n)]

    def compare_batch_device(self, surfaces: Sequence[dict], fmt, typ, ref_pixel_type, results: int, mask=None,
                             ssim: bool = False, stream: int = 0):
        """Device path of compare_batch.  surfaces: dicts with blocks, ref (device pointers as ints), width, height,
        ref_pitch_bytes and, optionally, block_errors (device pointer to floats) with block_errors_capacity.
        results: device pointer to len(surfaces) cfhip_compare_result.  stream 0 = the context's stream (the call
        then synchronises)."""
        n = len(surfaces)
        surf = (CompareSurface*max(n, 1))()
        for i, s in enumerate(surfaces):
            surf[i].blocks, surf[i].ref = int(s["blocks"]) or None, int(s["ref"]) or None
            surf[i].width, surf[i].height = s["width"], s["height"]
            surf[i].ref_pitch_bytes = s["ref_pitch_bytes"]
            if s.get("block_errors"):
                surf[i].block_errors = int(s["block_errors"])
                surf[i].block_errors_capacity = int(s.get("block_errors_capacity", 0))
        self._check(self._lib.cfhip_compare_batch_device(
            self._h, int(fmt), int(typ), surf, n, int(ref_pixel_type), self._mask(mask), COMPARE_SSIM if ssim else 0,
            _ptr(results), _stream(stream)))

    def rdo(self, payloads: Sequence[np.ndarray], sources: Sequence[np.ndarray], fmt, typ=Type.UNorm, lam: float = 1.0,
            max_sse_increase: Optional[int] = None, mask=None, row_above: bool = False,
            window_bytes: Optional[int] = None):
        """Rate-distortion optimisation of encoded payloads (cfhip_rdo): payloads[i] was encoded from sources[i],
        an (h, w, 4) uint8, float16 or float32 array.  Blocks are rewritten to copy byte ranges from the blocks before
        them where J = 16 SSE + round(16 lam) R falls (see include/cuttlefish_hip.h), no block's SSE rising by more
        than max_sse_increase (None: no cap).  All surfaces share one launch.  row_above: blocks may also copy from
        the block row above, on surfaces where that row lies within window_bytes (None: 32768) of the payload; either
        of the two arguments sends the call through cfhip_rdo_ex.  Returns (the optimised payloads, one
        dict of statistics per surface: blocks, blocks_changed, sse_before, sse_after, bits_before, bits_after)."""
        n = len(payloads)
        if len(sources) != n:
            raise ValueError("payloads and sources must list the same surfaces")
        entry, params = self._rdo_entry(False, lam, max_sse_increase, row_above, window_bytes)
        surf = (RdoSurface*max(n, 1))()
        srcs = [np.ascontiguousarray(s) for s in sources]
        if any(s.ndim != 3 or s.shape[2] != 4 for s in srcs):
            raise ValueError("sources must be (h, w, 4) uint8, float16 or float32")
        parts = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in payloads]
        outs = [np.empty_like(p) for p in parts]
        for i, (p, o, s) in enumerate(zip(parts, outs, srcs)):
            surf[i].blocks, surf[i].blocks_bytes = p.ctypes.data, p.nbytes
            surf[i].out, surf[i].out_capacity = o.ctypes.data, o.nbytes
            surf[i].height, surf[i].width = s.shape[:2]
            surf[i].pixels, surf[i].pixel_type, surf[i].row_pitch_bytes = s.ctypes.data, int(pixel_type_of(s)), s.strides[0]
        stats = (RdoStats*max(n, 1))()
        self._check(entry(self._h, int(fmt), int(typ), surf, n, ctypes.byref(params), self._mask(mask),
                          ctypes.addressof(stats)))
        return outs, [stats[i].as_dict() for i in range(n)]

    def _rdo_entry(self, device: bool, lam, max_sse_increase, row_above, window_bytes):
        """(the entry point, its parameters): the plain entry unless an option of cfhip_rdo_ex_params is given"""
        if row_above or window_bytes is not None:
            entry = self._lib.cfhip_rdo_ex_device if device else self._lib.cfhip_rdo_ex
            return entry, make_rdo_ex_params(lam, max_sse_increase, row_above, window_bytes)
        return (self._lib.cfhip_rdo_device if device else self._lib.cfhip_rdo), make_rdo_params(lam, max_sse_increase)

    def rdo_device(self, surfaces: Sequence[dict], fmt, typ, lam: float, stats: int,
                   max_sse_increase: Optional[int] = None, mask=None, stream: int = 0, row_above: bool = False,
                   window_bytes: Optional[int] = None):
        """Device path of rdo.  surfaces: dicts with blocks, out, pixels (device pointers as ints; out may equal
        blocks), out_capacity, width, height, pixel_type and row_pitch_bytes.  stats: device pointer to
        len(surfaces) cfhip_rdo_stats (overwritten).  stream 0 = the context's stream (the call then synchronises)."""
        n = len(surfaces)
        entry, params = self._rdo_entry(True, lam, max_sse_increase, row_above, window_bytes)
        surf = (RdoSurface*max(n, 1))()
        for i, s in enumerate(surfaces):
            surf[i].blocks, surf[i].out = int(s["blocks"]) or None, int(s["out"]) or None
            surf[i].out_capacity = int(s["out_capacity"])
            surf[i].width, surf[i].height = s["width"], s["height"]
            surf[i].pixels, surf[i].pixel_type = int(s["pixels"]) or None, int(s["pixel_type"])
            surf[i].row_pitch_bytes = s["row_pitch_bytes"]
        self._check(entry(
            self._h, int(fmt), int(typ), surf, n, ctypes.byref(params), self._mask(mask),
            _ptr(stats), _stream(stream)))

    def lz_size(self, payloads) -> dict:
        """The deflate-size estimate (cfhip_lz_size) of a byte stream: one array / bytes object, or a sequence of them
        taken as their concatenation.  Returns bytes_in, bits_q16, est_bytes, literals, matches, matched_bytes --
        the numbers of tests/lzsize_ref.py, exactly."""
        if isinstance(payloads, (bytes, bytearray, np.ndarray)):
            payloads = [payloads]
        parts = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray))
                 else np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in payloads]
        spans = (LzSpan*max(len(parts), 1))()
        for i, p in enumerate(parts):
            spans[i].bytes, spans[i].n = (p.ctypes.data if p.size else None), p.size
        out = LzStats()
        self._check(self._lib.cfhip_lz_size(self._h, spans, len(parts), ctypes.addressof(out)))
        return out.as_dict()

    def lz_size_device(self, spans: Sequence[tuple], out: int, stream: int = 0):
        """Device path of lz_size.  spans: (device pointer as int, bytes) pairs; out: device pointer to one
        cfhip_lz_stats (overwritten).  stream 0 = the context's stream (the call then synchronises)."""
        arr = (LzSpan*max(len(spans), 1))()
        for i, (ptr, n) in enumerate(spans):
            arr[i].bytes, arr[i].n = int(ptr) or None, int(n)
        self._check(self._lib.cfhip_lz_size_device(self._h, arr, len(spans), _ptr(out),
                                                   _stream(stream)))

    def lz_slice_bytes(self, nbytes: int = 0) -> int:
        """Set the slice the estimator cuts long streams into (whole blocks of 65536 bytes; 0: the default); returns
        the previous one.  Results do not depend on it; the context's scratch does."""
        return int(self._lib.cfhip_lz_slice_bytes(self._h, int(nbytes)))

    def _stage_ms(self, fn, names: tuple, takes_n: bool = False) -> dict:
        """One of the cfhip_*_stage_ms: kernel ms by stage name, in the stages' order"""
        ms = (ctypes.c_float*len(names))()
        self._check(fn(self._h, ms, len(names)) if takes_n else fn(self._h, ms))
        return dict(zip(names, (float(v) for v in ms)))

    def lz_stage_ms(self) -> dict:
        """Kernel ms of the last estimate's stages: keys, sort, match, parse, cost"""
        return self._stage_ms(self._lib.cfhip_lz_stage_ms, LZ_STAGES)

    def deflate(self, payloads) -> bytes:
        """The zlib stream (cfhip_deflate) of a byte stream: one array / bytes object, or a sequence of them taken as
        their concatenation.  zlib.decompress inverts it; the bytes are those of tests/deflate_ref.py, exactly.
        deflate_result() returns the call's cfhip_deflate_result."""
        if isinstance(payloads, (bytes, bytearray, np.ndarray)):
            payloads = [payloads]
        parts = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray))
                 else np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in payloads]
        spans = (LzSpan*max(len(parts), 1))()
        for i, p in enumerate(parts):
            spans[i].bytes, spans[i].n = (p.ctypes.data if p.size else None), p.size
        cap = deflate_bound(sum(p.size for p in parts))
        out = np.empty(cap, np.uint8)
        res = DeflateResult()
        self._check(self._lib.cfhip_deflate(self._h, spans, len(parts), out.ctypes.data, cap, ctypes.addressof(res)))
        self._deflate_result = res.as_dict()
        return out[:res.bytes_out].tobytes()

    def deflate_result(self) -> Optional[dict]:
        """The cfhip_deflate_result of the last deflate() on this context; None before the first one."""
        return getattr(self, "_deflate_result", None)

    def deflate_device(self, spans: Sequence[tuple], out: int, cap: int, result: int, stream: int = 0):
        """Device path of deflate.  spans: (device pointer as int, bytes) pairs; out: device pointer to cap bytes,
        4-byte aligned; result: device pointer to one cfhip_deflate_result (overwritten).  stream 0 = the context's
        stream (the call then synchronises)."""
        arr = (LzSpan*max(len(spans), 1))()
        for i, (ptr, n) in enumerate(spans):
            arr[i].bytes, arr[i].n = int(ptr) or None, int(n)
        self._check(self._lib.cfhip_deflate_device(
            self._h, arr, len(spans), _ptr(out), int(cap),
            _ptr(result), _stream(stream)))

    def deflate_stage_ms(self) -> dict:
        """Kernel ms of the last deflate's stages: keys, sort, match, parse, adler, codes, offsets, emit"""
        return self._stage_ms(self._lib.cfhip_deflate_stage_ms, DEFLATE_STAGES)

    def deflate_code_lengths(self, counts, limit: int) -> np.ndarray:
        """The device code builder alone (cfhip_deflate_code_lengths): one code length per count"""
        c = np.ascontiguousarray(counts, np.uint32)
        out = np.zeros(c.size, np.uint8)
        self._check(self._lib.cfhip_deflate_code_lengths(
            self._h, c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), c.size, int(limit),
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def deflate_indexed(self, payloads):
        """deflate() with the stream's index (cfhip_deflate_indexed): -> (the same bytes, the index as an (entries, 2)
        uint64 array of header_bit, token_bit per 4096 input bytes).  deflate_result() returns the call's result."""
        if isinstance(payloads, (bytes, bytearray, np.ndarray)):
            payloads = [payloads]
        parts = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray))
                 else np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in payloads]
        spans = (LzSpan*max(len(parts), 1))()
        for i, p in enumerate(parts):
            spans[i].bytes, spans[i].n = (p.ctypes.data if p.size else None), p.size
        total = sum(p.size for p in parts)
        cap = deflate_bound(total)
        out = np.empty(cap, np.uint8)
        index = np.zeros((zindex_entries(total), 2), np.uint64)
        res = DeflateResult()
        self._check(self._lib.cfhip_deflate_indexed(self._h, spans, len(parts), out.ctypes.data, cap,
                                                    index.ctypes.data if index.size else None, index.shape[0],
                                                    ctypes.addressof(res)))
        self._deflate_result = res.as_dict()
        return out[:res.bytes_out].tobytes(), index

    def deflate_indexed_device(self, spans: Sequence[tuple], out: int, cap: int, index: int, index_entries: int,
                               result: int, stream: int = 0):
        """Device path of deflate_indexed: deflate_device's arguments, and index: device pointer to index_entries
        cfhip_zindex_entry, 8-byte aligned."""
        arr = (LzSpan*max(len(spans), 1))()
        for i, (ptr, n) in enumerate(spans):
            arr[i].bytes, arr[i].n = int(ptr) or None, int(n)
        self._check(self._lib.cfhip_deflate_indexed_device(
            self._h, arr, len(spans), _ptr(out), int(cap),
            _ptr(index), int(index_entries),
            _ptr(result), _stream(stream)))

    def inflate(self, stream, index, n: int) -> bytes:
        """The n bytes of an indexed zlib stream (cfhip_inflate).  index: (entries, 2) integers, header_bit and token_bit
        per 4096 output bytes.  A stream or index that is invalid raises CfhipError with code E_DATA, the error class
        in .status and the lowest failing chunk in .bad_chunk.  inflate_result() returns the call's result either way."""
        z = np.frombuffer(bytes(stream), np.uint8)
        idx = np.ascontiguousarray(np.asarray(index, np.uint64).reshape(-1, 2))
        out = np.empty(int(n), np.uint8)
        res = InflateResult()
        # (an empty stream still passes a pointer: NULL is an argument error)
        zbuf = z if z.size else np.zeros(1, np.uint8)
        rc = self._lib.cfhip_inflate(self._h, zbuf.ctypes.data, z.size, idx.ctypes.data if idx.size else None,
                                     idx.shape[0], out.ctypes.data if out.size else None, out.size, ctypes.addressof(res))
        if rc == E_DATA:
            self._inflate_result = res.as_dict()
            raise CfhipError(rc, self._lib.cfhip_last_error(self._h).decode(), res.status, res.bad_chunk)
        self._check(rc)
        self._inflate_result = res.as_dict()
        return out.tobytes()

    def inflate_result(self) -> Optional[dict]:
        """The cfhip_inflate_result of the last inflate() on this context; None before the first one."""
        return getattr(self, "_inflate_result", None)

    def inflate_device(self, zstream: int, zbytes: int, index: int, index_entries: int, out: int, out_bytes: int,
                       result: int, stream: int = 0):
        """Device path of inflate.  zstream, index (8-byte aligned), out (4-byte aligned) and result (one
        cfhip_inflate_result, 8-byte aligned) are device pointers.  An invalid stream is reported through the result's
        status, not raised.  stream 0 = the context's stream (the call then synchronises)."""
        self._check(self._lib.cfhip_inflate_device(self._h, _ptr(zstream), int(zbytes), _ptr(index), int(index_entries),
                                                   _ptr(out), int(out_bytes), _ptr(result), _ptr(stream)))

    def inflate_stage_ms(self) -> dict:
        """Kernel ms of the last inflate's stages: decode, resolve, pack, fold"""
        return self._stage_ms(self._lib.cfhip_inflate_stage_ms, INFLATE_STAGES)

    def lz4_encode(self, payloads) -> bytes:
        """The LZ4 frame (cfhip_lz4_encode) of a byte stream: one array / bytes object, or a sequence of them taken as
        their concatenation.  The lz4 tool and LZ4F_decompress invert it, and so does lz4_decode; the bytes are those of
        tests/lz4_ref.py, exactly.  lz4_encode_result() returns the call's cfhip_lz4_result."""
        if isinstance(payloads, (bytes, bytearray, np.ndarray)):
            payloads = [payloads]
        parts = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray))
                 else np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in payloads]
        spans = (LzSpan*max(len(parts), 1))()
        for i, p in enumerate(parts):
            spans[i].bytes, spans[i].n = (p.ctypes.data if p.size else None), p.size
        cap = lz4_bound(sum(p.size for p in parts))
        out = np.empty(cap, np.uint8)
        res = Lz4Result()
        self._check(self._lib.cfhip_lz4_encode(self._h, spans, len(parts), out.ctypes.data, cap, ctypes.addressof(res)))
        self._lz4_encode_result = res.as_dict()
        return out[:res.bytes_out].tobytes()

    def lz4_encode_result(self) -> Optional[dict]:
        """The cfhip_lz4_result of the last lz4_encode() on this context; None before the first one."""
        return getattr(self, "_lz4_encode_result", None)

    def lz4_encode_device(self, spans: Sequence[tuple], out: int, cap: int, result: int, stream: int = 0):
        """Device path of lz4_encode.  spans: (device pointer as int, bytes) pairs; out: device pointer to cap bytes;
        result: device pointer to one cfhip_lz4_result (overwritten), 8-byte aligned.  stream 0 = the context's stream
        (the call then synchronises)."""
        arr = (LzSpan*max(len(spans), 1))()
        for i, (ptr, n) in enumerate(spans):
            arr[i].bytes, arr[i].n = int(ptr) or None, int(n)
        self._check(self._lib.cfhip_lz4_encode_device(
            self._h, arr, len(spans), _ptr(out), int(cap),
            _ptr(result), _stream(stream)))

    def lz4_encode_stage_ms(self) -> dict:
        """Kernel ms of the last lz4_encode's stages: keys, sort, match, parse, plan, offsets, emit, hash, final"""
        return self._stage_ms(self._lib.cfhip_lz4_encode_stage_ms, LZ4_ENCODE_STAGES, takes_n=True)

    def lz4_decode(self, frame, n: int) -> bytes:
        """The n bytes of one LZ4 frame (cfhip_lz4_decode): anyone's frame with independent blocks of at most 64 KiB.  A
        frame that is invalid, or valid but outside that (status LZ4_UNSUPPORTED: decode it on the host), raises
        CfhipError with code E_DATA, the class in .status and the lowest failing block in .bad_block.  A content
        checksum is not verified (lz4_decode_result()["content_checksum"] says whether one was there).
        lz4_decode_result() returns the call's result either way."""
        z = np.frombuffer(bytes(frame), np.uint8)
        out = np.empty(int(n), np.uint8)
        res = Lz4DecodeResult()
        zbuf = z if z.size else np.zeros(1, np.uint8)         # (an empty frame still passes a pointer)
        rc = self._lib.cfhip_lz4_decode(self._h, zbuf.ctypes.data, z.size, out.ctypes.data if out.size else None, out.size,
                                        ctypes.addressof(res))
        if rc == E_DATA:
            self._lz4_decode_result = res.as_dict()
            raise CfhipError(rc, self._lib.cfhip_last_error(self._h).decode(), res.status, res.bad_block)
        self._check(rc)
        self._lz4_decode_result = res.as_dict()
        return out.tobytes()

    def lz4_decode_result(self) -> Optional[dict]:
        """The cfhip_lz4_decode_result of the last lz4_decode() on this context; None before the first one."""
        return getattr(self, "_lz4_decode_result", None)

    def lz4_decode_device(self, frame: int, nbytes: int, out: int, out_bytes: int, result: int, stream: int = 0):
        """Device path of lz4_decode.  frame, out (4-byte aligned) and result (one cfhip_lz4_decode_result, 8-byte
        aligned) are device pointers.  An invalid frame is reported through the result's status, not raised.  stream 0 =
        the context's stream (the call then synchronises)."""
        self._check(self._lib.cfhip_lz4_decode_device(self._h, _ptr(frame), int(nbytes), _ptr(out), int(out_bytes),
                                                      _ptr(result), _ptr(stream)))

    def lz4_decode_stage_ms(self) -> dict:
        """Kernel ms of the last lz4_decode's stages: chain, blocks, final"""
        return self._stage_ms(self._lib.cfhip_lz4_decode_stage_ms, LZ4_DECODE_STAGES, takes_n=True)

    def png_encode(self, pixels: np.ndarray, color_type: int = PNG_RGBA, bit_depth: int = 8,
                   color_space=ColorSpace.Linear) -> bytes:
        """The PNG file (cfhip_png_encode) of an (h, w, 4) uint8 / float16 / float32 image, rows any pitch apart (a
        view of a wider image is taken as it is): colour type 0, 2, 4 or 6 at depth 8 or 16, an sRGB chunk for
        ColorSpace.sRGB.  Any PNG reader opens it; the bytes are those of tests/png_ref.py, exactly.  png_result()
        returns the call's cfhip_png_result."""
        a = np.asarray(pixels)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("expected an (h, w, 4) image, got shape %r" % (a.shape,))
        pt = pixel_type_of(a)
        if a.size and (a.strides[2] != a.itemsize or a.strides[1] != 4*a.itemsize or a.strides[0] < a.shape[1]*4*a.itemsize):
            a = np.ascontiguousarray(a)
        h, w = a.shape[:2]
        cap = png_bound(w, h, color_type, bit_depth, color_space)
        out = np.empty(max(cap, 1), np.uint8)
        res = PngResult()
        self._check(self._lib.cfhip_png_encode(self._h, a.ctypes.data if a.size else None, int(pt),
                                               a.strides[0] if a.size else 0, w, h, int(color_type), int(bit_depth),
                                               int(color_space), out.ctypes.data, cap, ctypes.addressof(res)))
        self._png_result = res.as_dict()
        return out[:res.bytes_out].tobytes()

    def png_result(self) -> Optional[dict]:
        """The cfhip_png_result of the last png_encode() on this context; None before the first one."""
        return getattr(self, "_png_result", None)

    def png_encode_device(self, pixels: int, pixel_type, pitch_bytes: int, width: int, height: int, out: int, cap: int,
                          result: int, color_type: int = PNG_RGBA, bit_depth: int = 8, color_space=ColorSpace.Linear,
                          stream: int = 0):
        """Device path of png_encode.  pixels: device pointer, aligned to the texel like pitch_bytes; out: device
        pointer to cap >= png_bound(...) bytes, any alignment; result: device pointer to one cfhip_png_result
        (overwritten; its bytes_out says where the file ends), 8-byte aligned.  stream 0 = the context's stream (the
        call then synchronises)."""
        self._check(self._lib.cfhip_png_encode_device(self._h, _ptr(pixels), int(pixel_type), int(pitch_bytes), int(width),
                                                      int(height), int(color_type), int(bit_depth), int(color_space),
                                                      _ptr(out), int(cap), _ptr(result), _ptr(stream)))

    def png_stage_ms(self) -> dict:
        """Kernel ms of the last png_encode's stages: filter, the zlib encoder's eight, crc, final"""
        return self._stage_ms(self._lib.cfhip_png_stage_ms, PNG_STAGES)

    def rdo_target(self, payloads: Sequence[np.ndarray], sources: Sequence[np.ndarray], fmt, typ=Type.UNorm,
                   target_ratio: float = 0.85, lam: float = 32.0, max_sse_increase: Optional[int] = None, mask=None,
                   row_above: bool = False, window_bytes: Optional[int] = None):
        """The rate-distortion pass to a target (cfhip_rdo_target): the smallest lambda <= lam (in steps of 1/16)
        whose payloads, concatenated, are estimated (lz_size) at no more than target_ratio x the estimate of the
        payloads as given; found by bisection on the device.  Returns (the payloads, one dict of statistics per
        surface, the result: lambda16, reached, trials, est_bytes_plain, est_bytes_final).  reached 0: even lam
        misses the target, and the pass at lam is returned."""
        n = len(payloads)
        if len(sources) != n:
            raise ValueError("payloads and sources must list the same surfaces")
        params = make_rdo_ex_params(lam, max_sse_increase, row_above, window_bytes)
        surf = (RdoSurface*max(n, 1))()
        srcs = [np.ascontiguousarray(s) for s in sources]
        if any(s.ndim != 3 or s.shape[2] != 4 for s in srcs):
            raise ValueError("sources must be (h, w, 4) uint8, float16 or float32")
        parts = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in payloads]
        outs = [np.empty_like(p) for p in parts]
        for i, (p, o, s) in enumerate(zip(parts, outs, srcs)):
            surf[i].blocks, surf[i].blocks_bytes = p.ctypes.data, p.nbytes
            surf[i].out, surf[i].out_capacity = o.ctypes.data, o.nbytes
            surf[i].height, surf[i].width = s.shape[:2]
            surf[i].pixels, surf[i].pixel_type, surf[i].row_pitch_bytes = s.ctypes.data, int(pixel_type_of(s)), s.strides[0]
        stats = (RdoStats*max(n, 1))()
        res = RdoTargetResult()
        self._check(self._lib.cfhip_rdo_target(self._h, int(fmt), int(typ), surf, n, ctypes.byref(params),
                                               self._mask(mask), ctypes.addressof(stats), float(target_ratio),
                                               ctypes.byref(res)))
        return outs, [stats[i].as_dict() for i in range(n)], res.as_dict()

    def rdo_target_device(self, surfaces: Sequence[dict], fmt, typ, target_ratio: float, lam: float, stats: int,
                          max_sse_increase: Optional[int] = None, mask=None, stream: int = 0, row_above: bool = False,
                          window_bytes: Optional[int] = None) -> dict:
        """Device path of rdo_target: the surfaces and stats of rdo_device (out may equal blocks: the pristine
        payloads are then kept in the context's scratch).  Blocks on either stream; returns the result dict."""
        n = len(surfaces)
        params = make_rdo_ex_params(lam, max_sse_increase, row_above, window_bytes)
        surf = (RdoSurface*max(n, 1))()
        for i, s in enumerate(surfaces):
            surf[i].blocks, surf[i].out = int(s["blocks"]) or None, int(s["out"]) or None
            surf[i].out_capacity = int(s["out_capacity"])
            surf[i].width, surf[i].height = s["width"], s["height"]
            surf[i].pixels, surf[i].pixel_type = int(s["pixels"]) or None, int(s["pixel_type"])
            surf[i].row_pitch_bytes = s["row_pitch_bytes"]
        res = RdoTargetResult()
        self._check(self._lib.cfhip_rdo_target_device(
            self._h, int(fmt), int(typ), surf, n, ctypes.byref(params), self._mask(mask),
            _ptr(stats), float(target_ratio), ctypes.byref(res),
            _stream(stream)))
        return res.as_dict()

    def unpack(self, payload: np.ndarray, fmt, typ, width: int, height: int) -> np.ndarray:
        """The payload of a standard (uncompressed) format, formats 1..28, back to texels on the GPU ->
        (height, width, 4) float32; channels the format does not store read 0, 0, 0, 1.  Raises (E_UNSUPPORTED) for
        block formats, PVRTC and illegal (format, type) pairs."""
        pixels = np.ascontiguousarray(payload, dtype=np.uint8)
        out = np.empty((height, width, 4), np.float32)
        self._check(self._lib.cfhip_std_unpack(self._h, int(fmt), int(typ), pixels.ctypes.data, pixels.nbytes, width,
                                               height, out.ctypes.data, out.nbytes))
        return out

    def unpack_device(self, pixels: int, fmt, typ, width: int, height: int, out: int, out_pitch_bytes: int,
                      stream: int = 0):
        """Device path of unpack: pixels (any alignment) / out (RGBA32F rows out_pitch_bytes apart, 4-byte aligned)
        are device pointers as ints.  stream 0 = the context's stream (the call then synchronises)."""
        self._check(self._lib.cfhip_std_unpack_device(
            self._h, int(fmt), int(typ), _ptr(pixels), width, height,
            _ptr(out), out_pitch_bytes, _stream(stream)))

    def compare_std(self, payload: np.ndarray, ref: np.ndarray, fmt, typ=Type.UNorm, mask=None,
                    ssim: bool = False) -> Comparison:
        """compare() for the standard formats: the payload's pixels, converted as unpack() converts them, against an
        (h, w, 4) uint8, float16 or float32 reference.  SSE and reference maxima for every type, log SSE for Float
        and UFloat, SSIM (ssim=True) for UNorm and SNorm (NaN otherwise).  No block error map."""
        ref = np.asarray(ref)
        pix = {np.dtype(np.uint8): PixelType.RGBA8, np.dtype(np.float32): PixelType.RGBA32F,
               np.dtype(np.float16): PixelType.RGBA16F}.get(ref.dtype)
        if ref.ndim != 3 or ref.shape[2] != 4 or pix is None:
            raise ValueError("reference must be (h, w, 4) uint8, float16 or float32")
        ref = np.ascontiguousarray(ref)
        h, w = ref.shape[:2]
        pixels = np.ascontiguousarray(payload, dtype=np.uint8)
        res = CompareResult()
        self._check(self._lib.cfhip_std_compare(
            self._h, int(fmt), int(typ), pixels.ctypes.data, pixels.nbytes, w, h, ref.ctypes.data, int(pix),
            ref.strides[0], self._mask(mask), COMPARE_SSIM if ssim else 0, ctypes.byref(res)))
        return Comparison(res, Layout.RGBA32F, None, typ=typ)

    def compare_std_device(self, pixels: int, fmt, typ, width: int, height: int, ref: int, ref_pixel_type,
                           ref_pitch_bytes: int, result: int, mask=None, ssim: bool = False, stream: int = 0):
        """Device path of compare_std: pixels / ref / result (one cfhip_compare_result) are device pointers as
        ints.  stream 0 = the context's stream (the call then synchronises)."""
        self._check(self._lib.cfhip_std_compare_device(
            self._h, int(fmt), int(typ), _ptr(pixels), width, height,
            _ptr(ref), int(ref_pixel_type), ref_pitch_bytes, self._mask(mask),
            COMPARE_SSIM if ssim else 0, _ptr(result),
            _stream(stream)))

    def last_kernel_ms(self) -> float:
        return float(self._lib.cfhip_last_kernel_ms(self._h))

    def profile_begin(self):
        self._check(self._lib.cfhip_profile_begin(self._h))

    def profile_end(self):
        """-> (summed kernel ms, launches) since profile_begin (hipEvents on the launch stream)."""
        ms, n = ctypes.c_float(), ctypes.c_uint32()
        self._check(self._lib.cfhip_profile_end(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def pinned_bytes(self) -> int:
        """page-locked host memory the context holds for its host path (source strip slots + payload landing ring)"""
        return int(self._lib.cfhip_pinned_bytes(self._h))

    def last_kernel_name(self) -> str:
        return self._lib.cfhip_last_kernel_name(self._h).decode()


def device_count() -> int:
    return int(load_library().cfhip_device_count())
