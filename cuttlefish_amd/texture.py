"""Host-side mirror of the reference interface for the block-encode path.

Mirrors ``cuttlefish::Texture`` as the reference's callers and tests use it
(lib/include/cuttlefish/Texture.h:42-836, lib/src/Texture.cpp):

    Texture(dimension, width, height, depth, mip_levels, color_space)   Texture::initialize :1136-1163
    dimension / width / height / depth / is_array / mip_level_count / face_count       :1170-1232
    set_image(image, [face,] mip, depth) / get_image([face,] mip, depth)              :1234-1318
    generate_mipmaps(filter, mip_levels, custom_mip_images)                          :1320-1514
    images_complete()                                                                :1516-1534
    convert(format, type, quality, alpha_type, color_mask, threads)                  :1536-1561
    converted / format / type / alpha_type / color_mask / data / data_size           :1563-1634
    save(file_name | None, file_type) -> SaveResult (or bytes)                       :1636-1685
    statics: is_format_valid, has_native_srgb, has_alpha, max_mipmap_levels, block_width /
             block_height / block_size, min_width / min_height, file_type,
             adjust_image_value_range                                              :318-1084

Same argument meaning and error behaviour: ``convert`` returns False when the images are
incomplete, the (format, type) pair is illegal (isFormatValid / createConverter returning nullptr,
Converter.cpp:339-412) or the texture is sRGB and the format has no native sRGB variant
(Texture::hasNativeSRGB, Texture.cpp:421-465); ``save`` returns the reference's SaveResult codes.

What runs where: the conversion is ONE call into the C-ABI (``cfhip_encode``) for all surfaces of
the texture -- every mip, array element, 3-D slice and cube face -- the whole-surface Converter of
INTEGRATION.md; mip generation runs on the GPU (``cfhip_generate_mips_device``,
``cfhip_generate_mips3d_device``, ``cfhip_resize_device``); the containers are serialised on the
host (containers.py).  Images are numpy arrays (h, w, 4): the reference's Image class, its loaders
and pixel operations are out of scope, so ``Image(format, w, h)`` of the
reference's tests is ``np.zeros((h, w, 4), np.float32)`` here.  The short form
``Texture(width, height, ...)`` of earlier rounds is kept (a 2-D texture).
"""
from __future__ import annotations

import enum
import io
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import api, containers
from .api import Alpha, ColorSpace, Format, Quality, Type

_NATIVE_SRGB = {Format.R8G8B8, Format.B8G8R8, Format.R8G8B8A8, Format.B8G8R8A8, Format.A8B8G8R8,
                Format.BC1_RGB, Format.BC1_RGBA, Format.BC2, Format.BC3, Format.BC7,
                Format.ETC2_R8G8B8, Format.ETC2_R8G8B8A1, Format.ETC2_R8G8B8A8} | \
    {Format(v) for v in range(43, 57)} | {Format(v) for v in range(57, 63)}     # ASTC, PVRTC (Texture.cpp:438-443)


class Dimension(enum.IntEnum):      # Texture::Dimension (Texture.h:48-54)
    Dim1D = 0
    Dim2D = 1
    Dim3D = 2
    Cube = 3


class CubeFace(enum.IntEnum):       # Texture::CubeFace (Texture.h:148-156)
    PosX = 0
    NegX = 1
    PosY = 2
    NegY = 3
    PosZ = 4
    NegZ = 5


class MipReplacement(enum.IntEnum):  # Texture::MipReplacement (Texture.h:172-176)
    Once = 0        # resume with the previous image when going down the mip chain
    Continue = 1    # continue with the new image


class FileType(enum.IntEnum):       # Texture::FileType (Texture.h:193-199)
    Auto = 0
    DDS = 1
    KTX = 2
    PVR = 3


class SaveResult(enum.IntEnum):     # Texture::SaveResult (Texture.h:204-211)
    Success = 0
    Invalid = 1
    UnknownFormat = 2
    Unsupported = 3
    WriteError = 4


class ImageFormat(enum.IntEnum):    # Image::Format (Image.h:54-74): only names an image's ORIGINAL storage here
    Invalid = 0
    Gray8 = 1
    Gray16 = 2
    RGB5 = 3
    RGB565 = 4
    RGB8 = 5
    RGB16 = 6
    RGBF = 7
    RGBA8 = 8
    RGBA16 = 9
    RGBAF = 10
    Int16 = 11
    UInt16 = 12
    Int32 = 13
    UInt32 = 14
    Float = 15
    Double = 16
    Complex = 17


class CustomMipImage:
    """Texture::CustomMipImage (Texture.h:330-395): an image that replaces a generated mip level."""

    def __init__(self, image, replacement: MipReplacement = MipReplacement.Once):
        self.image = image
        self.replacement = MipReplacement(replacement)


def image_index(*args) -> Tuple[int, int, int]:
    """Texture::ImageIndex (Texture.h:246-290): image_index([face,] mip=0, depth=0) -> the
    (face, mip, depth) key of a custom_mip_images dict."""
    if args and isinstance(args[0], CubeFace):
        face, rest = int(args[0]), args[1:]
    else:
        face, rest = 0, args
    mip = int(rest[0]) if len(rest) > 0 else 0
    depth = int(rest[1]) if len(rest) > 1 else 0
    return (face, mip, depth)


def _rgba8_of(image: np.ndarray) -> np.ndarray:
    """an image as RGBA8, quantised as the PVRTC encoder quantises float sources: round(clamp(f, 0, 1) * 255),
    NaN -> 0, in float32"""
    if image.dtype == np.uint8:
        return image
    f = image.astype(np.float32)
    f = np.minimum(np.where(f > 0, f, np.float32(0)), np.float32(1)).astype(np.float32)
    v = (f * np.float32(255)).astype(np.float32)
    r = np.floor(v)
    return (r + ((v - r) >= np.float32(0.5))).astype(np.uint8)


def _as_image(image) -> Optional[np.ndarray]:
    """What Image::convert(RGBAF) keeps of an image on this path: an (h, w, 4) array.  uint8 / float16
    arrays stay as they are (the kernels read them as the reference's RGBAF values, toColorBlock
    S3tcConverter.cpp:97-111 / HalfFloat.h), everything else becomes float32."""
    if image is None:
        return None
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 4 or image.shape[0] == 0 or image.shape[1] == 0:
        return None
    if image.dtype not in (np.uint8, np.float32, np.float16):
        image = image.astype(np.float32)
    return image


def _as_float32(image: np.ndarray) -> np.ndarray:
    """an image's texels as the kernels read them: uint8 as (float)(v / 255.0), float16 widened, float32 as stored"""
    if image.dtype == np.uint8:
        return (image.astype(np.float64)/255.0).astype(np.float32)
    return image.astype(np.float32, copy=False)


class Texture:
    allMipLevels = 0xFFFFFFFF   # Texture::allMipLevels (Texture.h:405)
    allCores = 0xFFFFFFFF       # Texture::allCores (:410); a thread count is meaningless on the GPU path

    # ---- statics (Texture.cpp:318-957) ---------------------------------------------------------
    @staticmethod
    def is_format_valid(format, type, file_type: Optional[FileType] = None) -> bool:
        """Texture::isFormatValid(format, type[, fileType]) (Texture.cpp:318-419)."""
        try:
            format, type = Format(format), Type(type)
            if format in api.PVRTC_FORMATS:
                if type != Type.UNorm:
                    return False
            else:
                api.query(format, type)
        except (ValueError, api.CfhipError):
            return False
        if file_type is None:
            return True
        file_type = FileType(file_type)
        if file_type == FileType.DDS:
            return (format, type) in containers._DXGI
        if file_type == FileType.KTX:
            return (format, type) in containers._GL or (format, type) in containers._GLU
        if file_type == FileType.PVR:
            return format in containers._PVR_GENERIC or format in containers._PVR_SPECIAL
        return False

    @staticmethod
    def has_native_srgb(format, type) -> bool:
        """Texture::hasNativeSRGB (Texture.cpp:421-465)."""
        try:
            return Format(format) in _NATIVE_SRGB and Type(type) == Type.UNorm
        except ValueError:
            return False

    @staticmethod
    def has_alpha(format) -> bool:
        return containers.has_alpha(format)

    @staticmethod
    def max_mipmap_levels(dimension, width: int, height: int, depth: int = 0) -> int:
        """Texture::maxMipmapLevels (Texture.cpp:514-527): 32 - clz of the largest extent."""
        big = max(int(width), int(height))
        if Dimension(dimension) == Dimension.Dim3D:
            big = max(big, int(depth))
        return int(big).bit_length()

    @staticmethod
    def _block(format, i) -> int:
        try:
            format = Format(format)
        except ValueError:
            return 0
        if format in api.PVRTC_FORMATS:
            return (4, 4, 8)[i]                     # Texture.cpp:596-773
        for t in Type:
            try:
                return api.query(format, t)[i]
            except api.CfhipError:
                continue
        return 0

    @staticmethod
    def block_width(format) -> int:
        return Texture._block(format, 0)

    @staticmethod
    def block_height(format) -> int:
        return Texture._block(format, 1)

    @staticmethod
    def block_size(format) -> int:
        return Texture._block(format, 2)

    @staticmethod
    def min_width(format) -> int:
        """Texture::minWidth (Texture.cpp:775-855): the block width of the formats of this backend; 8 for PVRTC1
        4 bpp, whose levels are never smaller than 2 x 2 blocks."""
        return 8 if Format(format) in api.PVRTC_FORMATS else Texture._block(format, 0)

    @staticmethod
    def min_height(format) -> int:
        return 8 if Format(format) in api.PVRTC_FORMATS else Texture._block(format, 1)

    @staticmethod
    def file_type(file_name: str) -> FileType:
        """Texture::fileType (Texture.cpp:939-957): by extension, case-insensitive."""
        low = str(file_name).lower()
        for ext, ft in ((".dds", FileType.DDS), (".ktx", FileType.KTX), (".pvr", FileType.PVR)):
            if low.endswith(ext):
                return ft
        return FileType.Auto

    @staticmethod
    def adjust_image_value_range(image, type, orig_image_format=ImageFormat.Invalid) -> Optional[np.ndarray]:
        """Texture::adjustImageValueRange (Texture.cpp:959-1084): what the reference's front end does
        to an image that came from an integer file format before a SNorm / UInt / Int conversion --
        SNorm remaps [0, 1] to [-1, 1] (v*2 - 1 in float), UInt scales to the original integer range
        (round(v*max)), Int also offsets by the type's minimum.  Images from float formats, and
        UNorm / UFloat / Float conversions, are returned unchanged.  image: (h, w, C) array; uint8 /
        uint16 arrays are read as v/255, v/65535 and name their own original format."""
        if image is None:
            return None
        image = np.asarray(image)
        fmt = ImageFormat(orig_image_format)
        if fmt == ImageFormat.Invalid:
            if image.dtype == np.uint8:
                fmt = {1: ImageFormat.Gray8, 3: ImageFormat.RGB8}.get(image.shape[-1], ImageFormat.RGBA8)
            elif image.dtype == np.uint16:
                fmt = {1: ImageFormat.Gray16, 3: ImageFormat.RGB16}.get(image.shape[-1], ImageFormat.RGBA16)
            else:
                fmt = ImageFormat.RGBAF
        if image.dtype == np.uint8:
            out = (image.astype(np.float64)/255.0).astype(np.float32)
        elif image.dtype == np.uint16:
            out = (image.astype(np.float64)/65535.0).astype(np.float32)
        else:
            out = image.astype(np.float32)
        type = Type(type)
        integer_origin = fmt in (ImageFormat.Gray8, ImageFormat.Gray16, ImageFormat.RGB5, ImageFormat.RGB565,
                                 ImageFormat.RGB8, ImageFormat.RGB16, ImageFormat.RGBA8, ImageFormat.RGBA16)
        if type not in (Type.SNorm, Type.UInt, Type.Int) or not integer_origin:
            return out if out is not image else out.copy()
        if type == Type.SNorm:
            return out*np.float32(2.0) - np.float32(1.0)
        if fmt in (ImageFormat.Gray8, ImageFormat.RGB8, ImageFormat.RGBA8):
            mul, off = [255.0]*4, [-128.0]*4
        elif fmt in (ImageFormat.Gray16, ImageFormat.RGB16, ImageFormat.RGBA16):
            mul, off = [65535.0]*4, [-32768.0]*4
        elif fmt == ImageFormat.RGB5:
            mul, off = [31.0, 31.0, 31.0, 0.0], [-16.0, -16.0, -16.0, 0.0]
        else:                                                    # RGB565
            mul, off = [31.0, 63.0, 31.0, 0.0], [-16.0, -32.0, -16.0, 0.0]
        c = out.shape[-1]
        m = np.array(mul[:c], np.float32)
        o = np.array(off[:c] if type == Type.Int else [0.0]*c, np.float32)
        v = out*m + o
        return (np.sign(v)*np.floor(np.abs(v) + np.float32(0.5))).astype(np.float32)    # std::round

    # ---- construction ---------------------------------------------------------------------------
    def __init__(self, *args, depth: int = 0, mip_levels: int = 1,
                 color_space: ColorSpace = ColorSpace.Linear, device_id: int = 0):
        """Texture(dimension, width, height, depth=0, mip_levels=1, color_space=Linear), the
        reference's constructor (Texture.h:536-538); Texture(width, height, depth=0, ...) is a 2-D
        texture; Texture() is invalid until initialize()."""
        self._device_id = device_id
        self._ctx: Optional[api.Context] = None
        self._valid = False
        self._reset_state()
        if not args:
            return
        if isinstance(args[0], Dimension):
            dimension, rest = args[0], list(args[1:])
        else:
            dimension, rest = Dimension.Dim2D, list(args)
        if len(rest) < 2:
            raise TypeError("Texture needs a width and a height")
        width, height = rest[0], rest[1]
        if len(rest) > 2:
            depth = rest[2]
        if len(rest) > 3:
            mip_levels = rest[3]
        if len(rest) > 4:
            color_space = rest[4]
        self.initialize(dimension, width, height, depth, mip_levels, color_space)

    def _reset_state(self):
        self._dim = Dimension.Dim2D
        self._w = self._h = self._depth = 0
        self._mips = 0
        self._faces = 0
        self._color_space = ColorSpace.Linear
        self._images: List[List[List[Optional[np.ndarray]]]] = []     # [mip][depth][face]
        self._textures: List[List[List[np.ndarray]]] = []
        self._format: Optional[Format] = None
        self._type: Optional[Type] = None
        self._alpha = Alpha.Standard
        self._mask = (True, True, True, True)
        self._rdo_stats = None
        self._rdo_target = None
        self._mip_post: List[List[dict]] = []
        self._bleed: List[dict] = []
        self._sdf: List[dict] = []
        self._spec_aa: List[dict] = []
        self._ao: List[dict] = []

    def initialize(self, dimension, width: int, height: int, depth: int = 0, mip_levels: int = 1,
                   color_space: ColorSpace = ColorSpace.Linear) -> bool:
        """Texture::initialize (Texture.cpp:1136-1163)."""
        self.reset()
        dimension = Dimension(dimension)
        width, height, depth = int(width), int(height), int(depth)
        if width <= 0 or height <= 0 or depth < 0 or (dimension == Dimension.Dim3D and depth == 0):
            return False
        self._valid = True
        self._dim, self._w, self._h, self._depth = dimension, width, height, depth
        self._color_space = ColorSpace(color_space)
        self._mips = min(max(int(mip_levels), 1), self.max_mipmap_levels(dimension, width, height, depth))
        self._faces = 6 if dimension == Dimension.Cube else 1
        # (the reference sizes every level of a 3-D texture with the BASE depth here, slots its own
        # setImage then refuses: levels are sized with depth(mip) instead)
        self._images = [[[None]*self._faces for _ in range(self.depth(m))] for m in range(self._mips)]
        return True

    def reset(self):
        self._valid = False
        self._reset_state()

    def is_valid(self) -> bool:
        return self._valid

    def __bool__(self) -> bool:
        return self._valid

    # ---- geometry (Texture.cpp:1170-1232) -----------------------------------------------------
    def dimension(self) -> Dimension:
        return self._dim

    def color_space(self) -> ColorSpace:
        return self._color_space

    def is_array(self) -> bool:
        return self._valid and self._dim != Dimension.Dim3D and self._depth > 0

    def width(self, mip: int = 0) -> int:
        if not self._valid or not (0 <= mip < self._mips):
            return 0
        return max(self._w >> mip, 1)

    def height(self, mip: int = 0) -> int:
        if not self._valid or not (0 <= mip < self._mips):
            return 0
        return max(self._h >> mip, 1)

    def depth(self, mip: int = 0) -> int:
        if not self._valid or not (0 <= mip < self._mips):
            return 0
        if self._dim == Dimension.Dim3D:
            return max(self._depth >> mip, 1)
        return max(self._depth, 1)

    def mip_level_count(self) -> int:
        return self._mips

    def face_count(self) -> int:
        return self._faces

    # ---- images (Texture.cpp:1234-1318) -------------------------------------------------------
    @staticmethod
    def _face_args(args):
        """([face,] mip=0, depth=0) -> (face or None, mip, depth)"""
        if args and isinstance(args[0], CubeFace):
            face, rest = args[0], args[1:]
        else:
            face, rest = None, args
        mip = int(rest[0]) if len(rest) > 0 else 0
        depth = int(rest[1]) if len(rest) > 1 else 0
        return face, mip, depth

    def _slot(self, face: Optional[CubeFace], mip: int, depth: int) -> Optional[int]:
        """face index of a legal ([face,] mip, depth) address, else None"""
        if not self._valid or mip < 0 or depth < 0 or depth >= self.depth(mip):
            return None
        if face is None:
            return 0 if self._faces == 1 else None
        if self._faces != 6 and face != CubeFace.PosX:
            return None
        return int(face)

    def get_image(self, *args) -> Optional[np.ndarray]:
        """Texture::getImage([face,] mip, depth): None is the reference's invalid Image."""
        face, mip, depth = self._face_args(args)
        f = self._slot(face, mip, depth)
        if f is None or mip >= len(self._images) or depth >= len(self._images[mip]):
            return None
        return self._images[mip][depth][f]

    def set_image(self, image, *args, mip: Optional[int] = None, depth: Optional[int] = None) -> bool:
        """Texture::setImage(image, [face,] mipLevel = 0, depth = 0): the image must have the
        level's size; it is kept as the reference's RGBAF conversion would present it."""
        face, m, d = self._face_args(args)
        m = m if mip is None else int(mip)
        d = d if depth is None else int(depth)
        if self._textures:
            return False
        f = self._slot(face, m, d)
        image = _as_image(image)
        if f is None or image is None:
            return False
        if image.shape[1] != self.width(m) or image.shape[0] != self.height(m):
            return False
        self._images[m][d][f] = image
        return True

    def images_complete(self) -> bool:
        if not self._valid:
            return False
        return all(im is not None for level in self._images for dep in level for im in dep)

    # ---- mip generation (Texture.cpp:1320-1514) -----------------------------------------------
    def _context(self) -> api.Context:
        if self._ctx is None:
            self._ctx = api.Context(self._device_id)
        return self._ctx

    def _to_device(self, image: np.ndarray):
        import torch  # device memory: plumbing only
        host = np.ascontiguousarray(image)
        return host, torch.from_numpy(host).to("cuda:%d" % self._device_id)

    def _resize(self, image: np.ndarray, w: int, h: int, filter) -> np.ndarray:
        """Image::resize(w, h, filter) -> RGBAF, on the GPU."""
        import torch
        host, src = self._to_device(image)
        dst = torch.empty((h, w, 4), dtype=torch.float32, device=src.device)
        self._context().resize_device(src.data_ptr(), api.pixel_type_of(host), host.shape[1], host.shape[0],
                                      host.strides[0], dst.data_ptr(), w, h,
                                      color_space=self._color_space, filter=int(filter))
        return dst.cpu().numpy()

    def _chain_2d(self, base: np.ndarray, levels: int, filter, post=None) -> List[np.ndarray]:
        """levels 1..levels-1 of one 2-D image, each from the one before; post = (alpha_coverage, normalize): the
        post-pass runs on the chain before it leaves the device"""
        import torch
        if levels <= 1:
            return []
        host, src = self._to_device(base)
        h, w = host.shape[:2]
        dsts = [torch.empty((max(1, h >> k), max(1, w >> k), 4), dtype=torch.float32, device=src.device)
                for k in range(1, levels)]
        self._context().generate_mips_device(src.data_ptr(), api.pixel_type_of(host), w, h, host.strides[0],
                                             [d.data_ptr() for d in dsts], color_space=self._color_space,
                                             filter=int(filter))
        if post is not None:
            self._post_device(host, src, dsts, post)
        return [d.cpu().numpy() for d in dsts]

    def _post_device(self, host: np.ndarray, src, dsts, post):
        """the mip post-pass on one chain's device buffers; its records join self._mip_post"""
        import torch
        res = torch.zeros((len(dsts), 4), dtype=torch.int32, device=src.device)
        self._context().mip_post_device([src.data_ptr()], api.pixel_type_of(host), host.shape[1], host.shape[0],
                                        host.strides[0], [[d.data_ptr() for d in dsts]], alpha_coverage=post[0],
                                        normalize=post[1], results=res.data_ptr() if post[0] is not None else 0)
        if post[0] is not None:
            rec = res.cpu().numpy().view(api.MIP_POST_RESULT_DTYPE).reshape(-1)
            self._mip_post.append([{k: r[k].item() for k in rec.dtype.names} for r in rec])

    def _post_images(self, base: np.ndarray, images: Sequence[np.ndarray], post) -> List[np.ndarray]:
        """the post-pass on levels that are on the host (a chain with custom mip images)"""
        import torch
        host, src = self._to_device(base)
        dsts = [torch.from_numpy(np.ascontiguousarray(im, dtype=np.float32)).to(src.device) for im in images]
        self._post_device(host, src, dsts, post)
        return [d.cpu().numpy() for d in dsts]

    def _level_3d(self, slices: Sequence[np.ndarray], filter) -> List[np.ndarray]:
        """the next level of a 3-D texture from the slices of one level: every slice resized in
        x, y, then generateMips3d along the depth (Texture.cpp:1384-1400, :103-227)"""
        import torch
        arrs = [np.asarray(s) for s in slices]
        if len({a.dtype for a in arrs}) > 1:
            # slices of mixed storage: every image becomes RGBAF first, as Image::convert does
            # (uint8 through v/255.0, Image.cpp:293-296) -- np.stack alone would promote 0..255
            arrs = [(a.astype(np.float64)/255.0).astype(np.float32) if a.dtype == np.uint8 else a.astype(np.float32)
                    for a in arrs]
        vol = np.ascontiguousarray(np.stack(arrs))
        src = torch.from_numpy(vol).to("cuda:%d" % self._device_id)
        d0, h0, w0 = vol.shape[:3]
        w, h, d = max(1, w0 >> 1), max(1, h0 >> 1), max(1, d0 >> 1)
        dst = torch.empty((d, h, w, 4), dtype=torch.float32, device=src.device)
        self._context().generate_mips3d_device(src.data_ptr(), api.pixel_type_of(vol[0]), w0, h0, d0,
                                               vol.strides[1], vol.strides[0], [dst.data_ptr()],
                                               color_space=self._color_space, filter=int(filter))
        out = dst.cpu().numpy()
        return [out[i] for i in range(d)]

    def generate_mipmaps(self, filter=api.ResizeFilter.CatmullRom, mip_levels: Optional[int] = None,
                         custom_mip_images: Optional[Dict[Tuple[int, int, int], CustomMipImage]] = None,
                         alpha_coverage: Optional[float] = None, normalize: Optional[str] = None) -> bool:
        """Texture::generateMipmaps(filter, mipLevels = allMipLevels, customMipImages)
        (Texture.cpp:1320-1514): every level from the previous one through Image::resize in linear
        space (3-D textures: also along the depth), on the GPU.  custom_mip_images maps
        image_index([face,] mip, depth) to a CustomMipImage that replaces the generated level --
        MipReplacement.Once resumes the generated chain below it, Continue builds the lower levels
        from the replacement.  Box / Linear: the reference's in-tree arithmetic; Cubic, CatmullRom
        (the default, as in the reference) and BSpline: FreeImage's resampler restated (FreeImage is
        absent: parity unpinned).  Generated levels are RGBAF (float32) images.

        alpha_coverage = t (0 < t <= 1) and normalize = "unorm" / "snorm" run the mip post-pass
        (Context.mip_post_device) on every surface's chain, custom mip images included, each against its own
        level 0: every level's alpha scaled so that its share of texels with alpha >= t matches level 0's, and every
        RGB renormalised as a normal ("unorm": create_normal_map's storage without KEEP_SIGN).  The pass scales alpha
        alone -- premultiplied colour is out of scope, so run it on straight alpha.  mip_post_results() returns the
        records.  3-D textures return False with either keyword: coverage of a volume is another definition.  With
        both left at None nothing changes."""
        if not self._valid or self._textures:
            return False
        post = None
        if alpha_coverage is not None or normalize is not None:
            if self._dim == Dimension.Dim3D or normalize not in (None, "unorm", "snorm"):
                return False
            if alpha_coverage is not None and not (0.0 < float(alpha_coverage) <= 1.0):
                return False
            post = (alpha_coverage, normalize)
        self._mip_post = []
        if any(im is None for dep in self._images[0] for im in dep):
            return False
        custom = dict(custom_mip_images or {})
        for c in custom.values():
            if c is None or _as_image(c.image) is None:
                return False
        try:
            filter = api.ResizeFilter(filter)
        except ValueError:
            return False
        if mip_levels is None:
            mip_levels = self.allMipLevels
        levels = min(max(int(mip_levels), 1),
                     self.max_mipmap_levels(self._dim, self._w, self._h, max(self._depth, 1)))
        base = self._images[0]
        if self._dim == Dimension.Dim3D:
            # if one slice of a level is replaced, all must be, with one replacement mode (:1362-1378)
            plan = []
            for mip in range(1, levels):
                md = max(self._depth >> mip, 1)
                has = [(0, mip, d) in custom for d in range(md)]
                if any(has) and not all(has):
                    return False
                customs = [custom[(0, mip, d)] for d in range(md)] if all(has) else []
                if any(c.replacement != customs[0].replacement for c in customs):
                    return False
                plan.append(customs)
            self._mips = levels
            images = [base] + [None]*(levels - 1)
            inputs: Optional[List[np.ndarray]] = None     # generated state kept under a `Once` replacement
            for mip in range(1, levels):
                mw, mh = self.width(mip), self.height(mip)
                customs = plan[mip - 1]
                restore = bool(customs) and customs[0].replacement == MipReplacement.Once and mip < levels - 1
                generated = None
                if not customs or restore:
                    source = inputs if inputs is not None else [dep[0] for dep in images[mip - 1]]
                    generated = self._level_3d(source, filter)
                inputs = generated if restore else None
                if customs:
                    level = [self._resize(_as_image(c.image), mw, mh, filter) for c in customs]
                else:
                    level = generated
                images[mip] = [[im] for im in level]
            self._images = images
            return True
        self._mips = levels
        depth = max(self._depth, 1)
        images = [base] + [[[None]*self._faces for _ in range(depth)] for _ in range(levels - 1)]
        for d in range(depth):
            for f in range(self._faces):
                keys = [(f, mip, d) in custom for mip in range(1, levels)]
                if not any(keys):
                    for mip, im in enumerate(self._chain_2d(base[d][f], levels, filter, post), start=1):
                        images[mip][d][f] = im
                    continue
                prev = None
                for mip in range(1, levels):
                    mw, mh = self.width(mip), self.height(mip)
                    c = custom.get((f, mip, d))
                    restore = c is not None and c.replacement == MipReplacement.Once
                    cur = None
                    if c is None or restore:
                        cur = self._resize(prev if prev is not None else images[mip - 1][d][f], mw, mh, filter)
                    prev = cur if restore else None
                    images[mip][d][f] = self._resize(_as_image(c.image), mw, mh, filter) if c is not None else cur
                if post is not None and levels > 1:
                    chain = [images[mip][d][f] for mip in range(1, levels)]
                    for mip, im in enumerate(self._post_images(base[d][f], chain, post), start=1):
                        images[mip][d][f] = im
        self._images = images
        return True

    def _stack_device(self, images):
        """images of one size and dtype, stacked and uploaded -> (the host stack, its device tensor, one device pointer
        per image)"""
        import torch
        stack = np.stack([np.ascontiguousarray(im) for im in images])
        dev = torch.from_numpy(stack).to("cuda:%d" % self._device_id)
        size = dev[0].numel()*dev.element_size()
        return stack, dev, [dev.data_ptr() + i*size for i in range(len(images))]

    def _in_place_pass(self, result_dtype, fields, call, beside: Optional["Texture"] = None):
        """A pass over every image currently set, each within itself: the images of equal size and dtype share one
        call(pointers, pixel type, width, height, row pitch, pointer to their 16-byte records) and are replaced by what
        it left in them.  -> the records in [mip][depth][face] order: mip, depth, face and `fields` of result_dtype.
        beside: a texture with an image of the same size wherever this one has one; those images are only read, their
        dtype splits the groups too, and call() takes (their pointers, pixel type, row pitch) as three more arguments."""
        import torch
        groups: Dict[tuple, List[Tuple[int, int, int]]] = {}
        for m, level in enumerate(self._images):
            for d, dep in enumerate(level):
                for f, im in enumerate(dep):
                    if im is not None:
                        other = () if beside is None else (beside._images[m][d][f].dtype.str,)
                        groups.setdefault((im.shape[0], im.shape[1], im.dtype.str) + other, []).append((m, d, f))
        records = {}
        for key, where in groups.items():
            h, w = key[:2]
            stack, dev, ptrs = self._stack_device([self._images[m][d][f] for m, d, f in where])
            res = torch.zeros((len(where), 4), dtype=torch.int32, device=dev.device)
            torch.cuda.current_stream(dev.device).synchronize()      # the context's stream does not wait for the fill
            if beside is None:
                call(ptrs, api.pixel_type_of(stack[0]), w, h, stack.strides[1], res.data_ptr())
            else:
                bstack, bdev, bptrs = self._stack_device([beside._images[m][d][f] for m, d, f in where])
                call(ptrs, api.pixel_type_of(stack[0]), w, h, stack.strides[1], res.data_ptr(), bptrs,
                     api.pixel_type_of(bstack[0]), bstack.strides[1])
            out = dev.cpu().numpy()
            rec = res.cpu().numpy().view(result_dtype).reshape(-1)
            for i, (m, d, f) in enumerate(where):
                self._images[m][d][f] = out[i]
                records[(m, d, f)] = dict(dict(mip=m, depth=d, face=f), **{k: int(rec[i][k]) for k in fields})
        return [records[k] for k in sorted(records)]

    def bleed_alpha(self, threshold: float = 0.0, wrap=False, max_distance: int = 0) -> bool:
        """Alpha bleeding (Context.alpha_bleed_device) of every image currently set -- all levels, depths and faces,
        each within itself: every texel with alpha <= threshold takes the colour of the nearest texel with
        alpha > threshold, bit for bit, alpha untouched.  Call it before generate_mipmaps / convert, so that the
        filters and the block encoders see a sensible colour under the transparent texels; it is for straight alpha,
        the alternative to premultiplication.  Images of equal size and dtype share one call.  wrap: a bool or (x, y)
        for tiling surfaces; max_distance: texels, 0 = unlimited.  bleed_results() returns the records.  False on
        an invalid or already converted texture, and on a 3-D texture: a volume's nearest seed is another
        definition."""
        if not self._valid or self._textures or self._dim == Dimension.Dim3D:
            return False
        self._bleed = self._in_place_pass(
            api.BLEED_RESULT_DTYPE, ("seeds", "filled", "max_dist2"),
            lambda ptrs, pt, w, h, pitch, res: self._context().alpha_bleed_device(ptrs, pt, w, h, pitch, threshold, wrap,
                                                                                  max_distance, res))
        return True

    def bleed_results(self):
        """The records of the last bleed_alpha(): one dict per image it ran on, in [mip][depth][face] order -- mip, depth,
        face, seeds, filled and max_dist2, the largest squared distance a colour travelled; [] before any call."""
        return [dict(r) for r in self._bleed]

    def alpha_distance_field(self, spread: int, threshold: float = 0.5, wrap=False, channels="a") -> bool:
        """A signed distance field (Context.alpha_sdf_device) in place of the alpha -- or of the named channels -- of
        every image currently set, all levels, depths and faces, each within itself and at its own size: texels with
        alpha > threshold are inside, and the channels take the Euclidean distance to the silhouette, exact up to `spread`
        texels, with 0.5 on the edge.  The intended order is the field first, then generate_mipmaps: a filtered distance
        is still a distance.  Do not pass alpha_coverage= to that generate_mipmaps: it would rescale an alpha that is no
        longer coverage.  Images of equal size and dtype share one call.  wrap: a bool or (x, y) for tiling surfaces.
        sdf_results() returns the records.  False on an invalid or already converted texture, and on a 3-D texture."""
        if not self._valid or self._textures or self._dim == Dimension.Dim3D:
            return False
        api.make_sdf_params(spread, 1, threshold, wrap, channels)
        self._sdf = self._in_place_pass(
            api.SDF_RESULT_DTYPE, ("inside", "saturated"),
            lambda ptrs, pt, w, h, pitch, res: self._context().alpha_sdf_device(ptrs, pt, w, h, pitch, ptrs, pt, pitch, spread, 1,
                                                                                threshold, wrap, channels, res))
        return True

    def sdf_results(self):
        """The records of the last alpha_distance_field(): one dict per image it ran on, in [mip][depth][face] order --
        mip, depth, face, inside (texels inside) and saturated (texels farther than the spread from the silhouette); []
        before any call."""
        return [dict(r) for r in self._sdf]

    def specular_antialias(self, normals: "Texture", channel="g", perceptual: bool = True, signed_normals: bool = False,
                           reconstruct_z: bool = False, variance_scale: float = 1.0, max_variance: float = 1.0) -> bool:
        """Specular anti-aliasing (Context.specular_aa_device) of this roughness -- or packed ORM -- texture against
        the normal map `normals`: call it after generate_mipmaps and before convert.  `channel` of every level from 1
        on, of every depth and face, takes sqrt of (the mean alpha^2 of the level-0 texels under the texel + the
        variance of the level-0 normals under it), so that what averaging the normals loses shows up as roughness.
        The value written replaces the mip filter's own value in that channel: it is the footprint mean of alpha^2
        plus the variance, not a correction of the filter's result.  Level 0, the other channels and `normals` are
        untouched; the levels become RGBAF (float32) images.  perceptual: the channel stores perceptual roughness
        (alpha = r^2); signed_normals / reconstruct_z: how `normals` stores its vectors; variance_scale 2 with
        max_variance 0.18 is the clamp of Kaplanyan et al.  `normals` may be this texture.  Surfaces of equal dtypes
        share one call.  specular_aa_results() returns the records.  False on an invalid, converted or 3-D texture, on
        `normals` of other dimensions, faces or depth, with an image missing, and with fewer than 2 levels."""
        import torch
        if not isinstance(normals, Texture) or not self._valid or self._textures or self._dim == Dimension.Dim3D:
            return False
        if not normals._valid or normals._textures or self._mips < 2:
            return False
        if (normals._dim, normals._w, normals._h, normals._depth, normals._faces) != \
                (self._dim, self._w, self._h, self._depth, self._faces):
            return False
        if any(im is None for level in self._images for dep in level for im in dep) or \
                any(im is None for dep in normals._images[0] for im in dep):
            return False
        api.make_spec_aa_params(channel, perceptual, signed_normals, reconstruct_z, 0.5, variance_scale, max_variance)
        device = "cuda:%d" % self._device_id
        per = self._mips - 1
        groups: Dict[tuple, List[Tuple[int, int]]] = {}
        for d, dep in enumerate(self._images[0]):
            for f, im in enumerate(dep):
                groups.setdefault((normals._images[0][d][f].dtype.str, im.dtype.str), []).append((d, f))
        records = {}
        for where in groups.values():
            n = len(where)
            nstack, ndev, nptrs = self._stack_device([normals._images[0][d][f] for d, f in where])
            rstack, rdev, rptrs = nstack, ndev, nptrs         # the normals' own surfaces when `normals` is this texture
            if normals is not self:
                rstack, rdev, rptrs = self._stack_device([self._images[0][d][f] for d, f in where])
            levels = [self._stack_device([_as_float32(np.ascontiguousarray(self._images[m][d][f])) for d, f in where])[1:]
                      for m in range(1, self._mips)]
            res = torch.zeros((n*per, 4), dtype=torch.int32, device=device)
            self._context().specular_aa_device(
                nptrs, api.pixel_type_of(nstack[0]), self._w, self._h, nstack.strides[1],
                [[levels[k][1][i] for k in range(per)] for i in range(n)], rough0=rptrs,
                rough_pixel_type=api.pixel_type_of(rstack[0]), rough_pitch=rstack.strides[1], channel=channel,
                perceptual=perceptual, signed_normals=signed_normals, reconstruct_z=reconstruct_z,
                variance_scale=variance_scale, max_variance=max_variance, results=res.data_ptr())
            rec = res.cpu().numpy().view(api.SPEC_AA_RESULT_DTYPE).reshape(n, per)
            for k in range(per):
                out = levels[k][0].cpu().numpy()
                for i, (d, f) in enumerate(where):
                    self._images[k + 1][d][f] = out[i]
                    r = rec[i][k]
                    records[(k + 1, d, f)] = dict(mip=k + 1, depth=d, face=f, clamped=int(r["clamped"]),
                                                  saturated=int(r["saturated"]),
                                                  max_added=float(np.uint32(r["max_added"]).view(np.float32)))
        self._spec_aa = [records[k] for k in sorted(records)]
        return True

    def specular_aa_results(self):
        """The records of the last specular_antialias(): one dict per level it wrote, in [mip][depth][face] order -- mip,
        depth, face, clamped (texels whose variance met max_variance), saturated (texels whose alpha^2 reached 1) and
        max_added (the largest variance added, after variance_scale); [] before any call."""
        return [dict(r) for r in self._spec_aa]

    def height_ambient_occlusion(self, heights: "Texture", channel="r", height_channel="r", *, radius: int,
                                 height: float = 1.0, directions: int = 16, strength: float = 1.0, bias: float = 0.0,
                                 uniform: bool = False, falloff: bool = False, wrap=False) -> bool:
        """Ambient occlusion from height maps (Context.height_ao_device): `channel` of every image currently set in
        this texture -- an occlusion or packed ORM texture -- takes the occlusion that the image of `heights` with the
        same [mip][depth][face] index casts on itself, its heights in `height_channel`, `height` texels per stored unit
        (the meaning the normal-map op's height has): the share of the sky the horizons within `radius` texels leave
        open, 1 on a flat surface.  The other channels and `heights` are untouched; the pixel types stay.  The intended
        order is the occlusion on level 0, then generate_mipmaps.  `heights` may be this texture: the height channel
        may then be overwritten.  Images of equal size and dtypes share one call.  directions: 8, 16 or 32; strength,
        bias, uniform, falloff: api.make_height_ao_params; wrap: a bool or (x, y) for tiling surfaces.  ao_results()
        returns the records.  False on an invalid, converted or 3-D texture, on `heights` of other dimensions, levels,
        faces or depth, and where `heights` lacks an image this texture has."""
        if not isinstance(heights, Texture) or not self._valid or self._textures or self._dim == Dimension.Dim3D:
            return False
        if not heights._valid or heights._textures:
            return False
        if (heights._dim, heights._w, heights._h, heights._depth, heights._faces, heights._mips) != \
                (self._dim, self._w, self._h, self._depth, self._faces, self._mips):
            return False
        for level, hlevel in zip(self._images, heights._images):
            for dep, hdep in zip(level, hlevel):
                for im, him in zip(dep, hdep):
                    if im is not None and (him is None or him.shape != im.shape):
                        return False
        kw = dict(radius=radius, height_scale=height, directions=directions, channel=height_channel, channels=channel,
                  strength=strength, bias=bias, uniform=uniform, falloff=falloff, wrap=wrap)
        api.make_height_ao_params(**kw)
        ctx = self._context()
        if heights is self:
            call = lambda ptrs, pt, w, h, pitch, res: ctx.height_ao_device(          # noqa: E731
                ptrs, pt, w, h, pitch, ptrs, pt, pitch, results=res, **kw)
            records = self._in_place_pass(api.HEIGHT_AO_RESULT_DTYPE, ("occluded", "darkest"), call)
        else:
            call = lambda ptrs, pt, w, h, pitch, res, hptrs, hpt, hpitch: ctx.height_ao_device(      # noqa: E731
                hptrs, hpt, w, h, hpitch, ptrs, pt, pitch, results=res, **kw)
            records = self._in_place_pass(api.HEIGHT_AO_RESULT_DTYPE, ("occluded", "darkest"), call, beside=heights)
        for r in records:
            r["darkest"] = float(np.uint32(r["darkest"]).view(np.float32))
        self._ao = records
        return True

    def ao_results(self):
        """The records of the last height_ambient_occlusion(): one dict per image it ran on, in [mip][depth][face] order
        -- mip, depth, face, occluded (texels with a horizon above the bias) and darkest (the smallest value stored, as
        a float); [] before any call."""
        return [dict(r) for r in self._ao]

    # ---- environment maps (Context.equirect_to_cube / cube_prefilter / cube_sh9) ------------------------------------
    @staticmethod
    def from_panorama(image, face_size: int, supersample: int = 2, color_space: ColorSpace = ColorSpace.Linear,
                      device_id: int = 0) -> Optional["Texture"]:
        """A Dimension.Cube texture of face_size^2 faces with level 0 set from an equirectangular panorama (an
        (h, w, 4) uint8 / float16 / float32 array or an Image), resampled on the GPU with supersample^2 fetches per texel.
        The texels are read as stored; color_space only names the space of the texture made.  The panorama's centre
        column looks along +Z and its top row along +Y.  None for what is no image."""
        pixels = _as_image(getattr(image, "pixels", image))
        if pixels is None:
            return None
        t = Texture(Dimension.Cube, int(face_size), int(face_size), 0, 1, color_space, device_id=device_id)
        if not t.is_valid():
            return None
        for f, face in enumerate(t._context().equirect_to_cube(pixels, int(face_size), supersample)):
            t.set_image(face, CubeFace(f), 0)
        return t

    def _cube_faces(self) -> Optional[List[np.ndarray]]:
        """level 0 of a cube that is not an array, not converted and has its six faces; else None"""
        if not self._valid or self._textures or self._dim != Dimension.Cube or self._depth > 0 or self._w != self._h:
            return None
        faces = self._images[0][0]
        if any(im is None for im in faces):
            return None
        return [_as_float32(im) for im in faces]

    def prefilter_environment(self, mip_levels: Optional[int] = None, samples: int = 256,
                              roughness: Optional[Sequence[float]] = None) -> bool:
        """The specular chain of an environment cube in place of generate_mipmaps: level k becomes level 0 convolved
        with a GGX lobe of roughness r_k (Context.cube_prefilter: a Box chain on the device, then `samples` samples per
        texel, a multiple of 64 from 64 to 4096).  mip_levels: all by default; roughness: one value in [0, 1] per level,
        by default r_k = k / (K - 1), 0 -- a copy -- for a single level.  The levels are RGBAF (float32) images.  False,
        before any device work, for a texture that is no cube, is an array, is converted or lacks a face of level 0."""
        plan = self._prefilter_plan(mip_levels, roughness)
        if plan is None:
            return False
        faces, levels, roughness = plan
        self._set_cube_chain(self._context().cube_prefilter(faces, roughness, samples), levels)
        return True

    def _prefilter_plan(self, mip_levels, roughness):
        """what prefilter_environment and prefilter_lobe work from: (the faces of level 0, the level count, one roughness
        or None per level), or None for their refusals"""
        faces = self._cube_faces()
        if faces is None:
            return None
        full = api.cube_level_count(self._w)
        levels = full if mip_levels is None else min(max(int(mip_levels), 1), full)
        if roughness is None:
            roughness = [0.0] if levels == 1 else [k/float(levels - 1) for k in range(levels)]
        roughness = [None if r is None else float(r) for r in roughness]
        if len(roughness) != levels or any(r is not None and not (0.0 <= r <= 1.0) for r in roughness):
            return None
        return faces, levels, roughness

    def _set_cube_chain(self, chain, levels: int):
        self._mips = levels
        self._images = [[[chain[k][f] for f in range(6)]] for k in range(levels)]

    def irradiance_sh9(self) -> Optional[np.ndarray]:
        """The nine spherical-harmonic coefficients of level 0 of an environment cube, (9, 4) float64 in the order 1, y,
        z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2 (Context.cube_sh9); api.sh9_irradiance evaluates the diffuse term from
        them.  None where prefilter_environment returns False."""
        faces = self._cube_faces()
        if faces is None:
            return None
        return self._context().cube_sh9(faces)[0]

    # ---- the rest of a split-sum shader's inputs (Context.brdf_lut / cube_prefilter_lobe / cube_irradiance) -----------
    @staticmethod
    def brdf_lut(size: int = 128, samples: int = 1024, sheen: bool = False, device_id: int = 0) -> Optional["Texture"]:
        """The BRDF lookup table of the split sum as a 2-D size^2 RGBAF texture, ready for convert (a 16-bit float
        standard format is the usual choice): x is N.V, y roughness, R and G the scale and bias of F0 under GGX, B the
        Charlie sheen albedo when `sheen` (else 0), A 1 (Context.brdf_lut).  None for a size outside 1 to 1024."""
        if isinstance(size, (bool, np.bool_)) or not isinstance(size, (int, np.integer)) or not 1 <= size <= api.ENV_MAX_LUT:
            return None
        t = Texture(int(size), int(size), device_id=device_id)
        if not t.is_valid():
            return None
        t.set_image(t._context().brdf_lut(int(size), int(size), samples, sheen))
        return t

    def prefilter_lobe(self, kind: int, mip_levels: Optional[int] = None, samples: int = 256,
                       roughness: Optional[Sequence[float]] = None) -> bool:
        """prefilter_environment under another lobe: api.LOBE_CHARLIE for a sheen chain, api.LOBE_LAMBERT for the
        irradiance over pi in every level (its roughness is not read: every level but a None entry is filtered),
        api.LOBE_GGX for prefilter_environment itself.  The same levels, defaults and refusals, and one more: False
        where a Charlie level is so sharp that none of `samples` records stays above the horizon
        (Context.cube_prefilter_lobe; the default levels of a chain want 1024 samples)."""
        if kind not in (api.LOBE_GGX, api.LOBE_CHARLIE, api.LOBE_LAMBERT):
            return False
        plan = self._prefilter_plan(mip_levels, roughness)
        if plan is None:
            return False
        faces, levels, roughness = plan
        api._check_samples(samples)                        # raises as prefilter_environment does
        try:
            chain = self._context().cube_prefilter_lobe(faces, kind, roughness, samples)
        except ValueError:                                 # a level with no record above the horizon
            return False
        self._set_cube_chain(chain, levels)
        return True

    def irradiance_cube(self, face_size: int = 32, method: str = "sh9", samples: int = 1024) -> Optional["Texture"]:
        """A new one-level cube of face_size^2 RGBAF faces holding the irradiance of this cube's level 0 over pi -- what
        a shader multiplies by the albedo.  method "sh9": the nine coefficients and their evaluation, both on the device
        (Context.cube_sh9_device, cube_irradiance_device), any face_size.  method "lambert": `samples` uniform
        directions per texel weighted by the cosine, through the prefilter kernel; face_size must be this cube's size
        halved some number of times, and the levels above the wanted one are made as copies and dropped -- accepted
        for a pass that runs once per environment.  None where prefilter_environment returns False, and for another
        method or such a face_size."""
        import torch
        faces = self._cube_faces()
        if faces is None or method not in ("sh9", "lambert") or isinstance(face_size, (bool, np.bool_)) \
                or not isinstance(face_size, (int, np.integer)) or not 1 <= face_size <= api.ENV_MAX_FACE:
            return None
        n, m = self._w, int(face_size)
        if method == "lambert":
            k = next((k for k in range(api.cube_level_count(n)) if max(1, n >> k) == m), None)
            if k is None:
                return None
        ctx = self._context()
        if method == "lambert":
            level = ctx.cube_prefilter_lobe(faces, api.LOBE_LAMBERT, [None]*k + [1.0], samples)[k]
        else:
            device = "cuda:%d" % self._device_id
            dev = torch.from_numpy(np.ascontiguousarray(np.stack(faces), dtype=np.float32)).to(device)
            res = torch.zeros(37, dtype=torch.float64, device=device)
            out = torch.empty((6, m, m, 4), dtype=torch.float32, device=device)
            ctx.cube_sh9_device([dev[f].data_ptr() for f in range(6)], n, res.data_ptr())
            ctx.cube_irradiance_device(res.data_ptr(), [out[f].data_ptr() for f in range(6)], m, over_pi=True)
            level = out.cpu().numpy()
        t = Texture(Dimension.Cube, m, m, 0, 1, self._color_space, device_id=self._device_id)
        t._ctx = self._ctx
        for f in range(6):
            t.set_image(level[f], CubeFace(f), 0)
        return t

    def mip_post_results(self):
        """The records of the last generate_mipmaps(alpha_coverage=...): one list per surface in [depth][face] order,
        one dict per generated level (scale, target, count_before, count_after); [] when coverage was not asked."""
        return [list(r) for r in self._mip_post]

    # ---- conversion (Texture.cpp:1536-1561) ----------------------------------------------------
    def convert(self, format: Format, type: Type, quality: Quality = Quality.Normal,
                alpha_type: Alpha = Alpha.Standard,
                color_mask: Sequence[bool] = (True, True, True, True),
                threads: int = allCores) -> bool:
        del threads  # the GPU path has no thread count (PvrtcConverter-style whole surface)
        if not self.images_complete() or not self.is_format_valid(format, type):
            return False
        format, type = Format(format), Type(type)
        if self._color_space == ColorSpace.sRGB and not self.has_native_srgb(format, type):
            return False
        params = api.make_params(format, type, quality, alpha_type, color_mask, self._color_space)
        flat = [im for level in self._images for dep in level for im in dep]
        # the reference converts every image to RGBAF before it reaches a converter
        # (Converter.h:52-56): half-float images are bit-exact sources for BC6H and the
        # uncompressed packers, every other block kernel takes them as floats
        if not (format == Format.BC6H or int(format) < int(Format.BC1_RGB)):
            flat = [im.astype(np.float32) if im.dtype == np.float16 else im for im in flat]
        try:
            if format in api.PVRTC_FORMATS:
                # PVRTC1 block order is defined for power-of-two grids only: other sizes are refused
                if any(im.shape[0] & (im.shape[0] - 1) or im.shape[1] & (im.shape[1] - 1) for im in flat):
                    return False
                flat = [im.astype(np.float32) if im.dtype == np.float16 else im for im in flat]
                outs = self._context().encode_pvrtc(flat, params)
            else:
                outs = self._context().encode(flat, params)
        except api.CfhipError as e:
            if e.code == api.E_UNSUPPORTED:
                return False  # createConverter -> nullptr -> convert() returns false
            raise
        it = iter(outs)
        self._textures = [[[next(it) for _ in dep] for dep in level] for level in self._images]
        # Converter::convert frees each source image once its surface is done (:586)
        self._images = [[[None]*len(dep) for dep in level] for level in self._images]
        self._format, self._type = format, type
        self._alpha, self._mask = Alpha(alpha_type), tuple(bool(m) for m in color_mask)
        return True

    @staticmethod
    def load(file_name_or_bytes, file_type: FileType = FileType.Auto, format=None, type=None,
             device_id: int = 0) -> Optional["Texture"]:
        """A converted texture from a DDS / KTX / PVR file (a path or its bytes), None where it cannot be read.
        format / type select another member of a collision set (containers.read_texture).  For a file this
        project wrote, load(b).save_bytes(same type) returns b."""
        data = file_name_or_bytes
        try:
            if not isinstance(data, (bytes, bytearray, memoryview)):
                if FileType(file_type) == FileType.Auto:
                    file_type = Texture.file_type(str(data))
                with open(data, "rb") as f:
                    data = f.read()
            tf = containers.read_texture(data, int(file_type), format=format, type=type)
        except (OSError, ValueError):
            return None
        dim = {"1d": Dimension.Dim1D, "2d": Dimension.Dim2D, "3d": Dimension.Dim3D, "cube": Dimension.Cube}[tf.dimension]
        t = Texture(device_id=device_id)
        if not t.initialize(dim, tf.width, tf.height, tf.depth, tf.levels, tf.color_space):
            return None
        # one buffer, the surfaces views of it in storage order: a batched decode then uploads them as one copy
        blob = np.frombuffer(b"".join(f for level in tf.surfaces for dep in level for f in dep), np.uint8)
        offs = np.cumsum([0] + [len(f) for level in tf.surfaces for dep in level for f in dep])
        it = iter(range(len(offs) - 1))
        t._textures = [[[blob[offs[i]:offs[i + 1]] for i in (next(it) for _ in dep)] for dep in level]
                       for level in tf.surfaces]
        t._format, t._type, t._alpha = tf.fmt, tf.typ, tf.alpha
        return t

    def converted(self) -> bool:
        return bool(self._textures)

    def format(self) -> Optional[Format]:
        return self._format

    def type(self) -> Optional[Type]:
        return self._type

    def alpha_type(self) -> Alpha:
        return self._alpha

    def color_mask(self):
        return self._mask

    def data(self, *args) -> Optional[np.ndarray]:
        """Texture::data([face,] mipLevel = 0, depth = 0): the payload bytes, None where the reference
        returns nullptr."""
        face, mip, depth = self._face_args(args)
        if not self._textures:
            return None
        f = self._slot(face, mip, depth)
        if f is None or mip >= len(self._textures):
            return None
        return self._textures[mip][depth][f]

    def data_size(self, *args) -> int:
        d = self.data(*args)
        return 0 if d is None else int(d.nbytes)

    def compare(self, source: "Texture", ssim: bool = True):
        """Quality of this converted texture against `source`, an unconverted texture of the same dimension, size,
        mip levels, depth and faces (convert() frees a texture's own images).  Returns (one api.Comparison per
        surface in (mip, depth, face) order, the pooled PSNR over every surface).  The channels compared are the
        colour mask's, without alpha when the alpha type is None or the format has none.  Standard formats go through
        Context.compare_std: the same return shape, SSIM NaN for the types that are not normalised."""
        if not self._textures:
            raise ValueError("compare: this texture is not converted")
        if source is self or not source.images_complete():
            raise ValueError("compare: source must be a separate texture holding every image")
        if (source.dimension(), source.width(), source.height(), source.depth(), source.mip_level_count(),
                source.face_count()) != (self._dim, self.width(), self.height(), self.depth(), self.mip_level_count(),
                                         self.face_count()):
            raise ValueError("compare: source differs in dimension, size, depth, mip levels or faces")
        mask = list(self._mask)
        if self._alpha == Alpha.None_ or not self.has_alpha(self._format):
            mask[3] = False
        ctx = self._context()
        if self._format in api.PVRTC_FORMATS:
            return self._compare_pvrtc(ctx, source, mask, ssim)
        # the standard formats have their own entry (cfhip_std_compare): SSIM is NaN for the non-normalised types.
        # Their texels are floats, so an 8-bit source is measured as the RGBAF image the converter read
        # (float(v/255), Image.cpp:293-296): a lossless conversion then compares equal, PSNR inf.
        std = int(self._format) < int(Format.BC1_RGB)
        flat = self._flat()
        refs = [source._images[m][d][f] for m, d, f, _ in flat]
        if std:
            results = []
            for (_, _, _, payload), ref in zip(flat, refs):
                if ref.dtype == np.uint8:
                    ref = (ref.astype(np.float64)/255.0).astype(np.float32)
                results.append(ctx.compare_std(payload, ref, self._format, self._type, mask=mask, ssim=ssim))
        else:
            # one batched call per reference dtype (cfhip_compare_batch measures one pixel type per call)
            results = [None]*len(flat)
            for dt in sorted({r.dtype for r in refs}, key=str):
                idx = [i for i, r in enumerate(refs) if r.dtype == dt]
                got = ctx.compare_batch([flat[i][3] for i in idx], [refs[i] for i in idx], self._format, self._type,
                                        mask=mask, ssim=ssim)
                for i, r in zip(idx, got):
                    results[i] = r
        return results, self._pooled(results)

    @staticmethod
    def _pooled(results) -> float:
        """the pooled PSNR of compare(): over every surface and compared channel"""
        sse = sum(sum(r.sse[c] for c in r.compared()) for r in results)
        n = sum(r.texels * len(r.compared()) for r in results)
        if n == 0:
            raise ValueError("compare: no channel compared")
        peak = max(r.peak() for r in results)
        return float("inf") if sse == 0.0 else 10.0 * float(np.log10(peak * peak * n / sse))

    @staticmethod
    def _pooled_pvrtc(results, texels: int, chans) -> float:
        sse = sum(r[c] for r in results for c in chans)
        return float("inf") if sse == 0 else 10.0 * float(np.log10(255.0 * 255.0 * texels * len(chans) / sse))

    def _measure_device(self, ctx, format, type, items, mask, ssim):
        """Quality of device payloads against device texels, without a copy through the host.  items: one
        (payload tensor, texel tensor, PixelType, width, height) per surface, the texels tightly pitched.  Block
        formats: one Context.compare_batch_device call per pixel type; standard formats and PVRTC: their
        per-surface device entries (an RGBA8 reference of a standard format is first widened on the device to the
        RGBAF image the converter read, as compare() widens it on the host; a float reference of PVRTC is
        quantised on the host as compare() quantises it: PVRTC's fused SSE reads RGBA8 alone).  Returns what
        compare() returns per surface."""
        import ctypes
        import torch
        dev = "cuda:%d" % self._device_id
        tb = {api.PixelType.RGBA8: 4, api.PixelType.RGBA32F: 16, api.PixelType.RGBA16F: 8}
        n = len(items)
        if format in api.PVRTC_FORMATS:
            sums = torch.empty((n, 4), dtype=torch.int64, device=dev)
            host = {}
            for i, (pay, tex, pt, w, h) in enumerate(items):
                if pt == api.PixelType.RGBA8:
                    ctx.decode_pvrtc_sse_device(pay.data_ptr(), format, w, h, tex.data_ptr(), w*4,
                                                sums[i].data_ptr(), type)
                else:
                    dt = np.float32 if pt == api.PixelType.RGBA32F else np.float16
                    ref = _rgba8_of(tex.cpu().numpy().view(dt).reshape(h, w, 4))
                    host[i] = ctx.decode_pvrtc_sse(pay.cpu().numpy(), ref, format, type)
            got = sums.cpu().numpy().astype(np.uint64)
            return [host[i] if i in host else [int(v) for v in got[i]] for i in range(n)]
        size = ctypes.sizeof(api.CompareResult)
        raw = np.empty((n, size), np.uint8)
        if int(format) < int(Format.BC1_RGB):
            res = torch.empty(n*size, dtype=torch.uint8, device=dev)
            for i, (pay, tex, pt, w, h) in enumerate(items):
                ref, rp = tex, pt
                if pt == api.PixelType.RGBA8:
                    ref, rp = torch.empty((h, w, 4), dtype=torch.float32, device=dev), api.PixelType.RGBA32F
                    ctx.image_ops_device(tex.data_ptr(), pt, w, h, w*4, api.make_image_ops(), ref.data_ptr(), w*16)
                ctx.compare_std_device(pay.data_ptr(), format, type, w, h, ref.data_ptr(), rp, w*tb[rp],
                                       res.data_ptr() + i*size, mask=mask, ssim=ssim)
            raw[:] = res.cpu().numpy().reshape(n, size)
            layout = api.Layout.RGBA32F
        else:
            for pt in sorted({int(it[2]) for it in items}):
                idx = [i for i, it in enumerate(items) if int(it[2]) == pt]
                res = torch.empty(len(idx)*size, dtype=torch.uint8, device=dev)
                ctx.compare_batch_device([dict(blocks=items[i][0].data_ptr(), ref=items[i][1].data_ptr(),
                                               width=items[i][3], height=items[i][4],
                                               ref_pitch_bytes=items[i][3]*tb[api.PixelType(pt)]) for i in idx],
                                         format, type, pt, res.data_ptr(), mask=mask, ssim=ssim)
                raw[idx] = res.cpu().numpy().reshape(len(idx), size)
            layout, _ = api.decoded_layout(format, type)
        std = layout == api.Layout.RGBA32F
        return [api.Comparison(api.CompareResult.from_buffer_copy(raw[i].tobytes()), layout, None,
                               typ=type if std else None) for i in range(n)]

    def _encode_resident(self, ctx, flat, format, type, params):
        """Upload every image once and encode it from there (Context.encode_device): (the host arrays, their device
        copies, the device payloads), or None where the encoder answers UNSUPPORTED."""
        import torch
        dev = "cuda:%d" % self._device_id
        pvrtc = format in api.PVRTC_FORMATS
        hosts = [np.ascontiguousarray(im) for im in flat]
        texels = [torch.from_numpy(h).to(dev) for h in hosts]
        size = api.pvrtc_payload_size if pvrtc else api.payload_size
        try:
            pays = [torch.empty(size(format, type, h.shape[1], h.shape[0]), dtype=torch.uint8, device=dev) for h in hosts]
            surfaces = [dict(pixels=t.data_ptr(), pixel_type=int(api.pixel_type_of(h)), width=h.shape[1],
                             height=h.shape[0], row_pitch_bytes=h.strides[0], out=p.data_ptr(), out_capacity=p.numel())
                        for h, t, p in zip(hosts, texels, pays)]
            # one call per pixel type, as transcode() encodes
            for pt in sorted({s["pixel_type"] for s in surfaces}):
                group = [s for s in surfaces if s["pixel_type"] == pt]
                (ctx.encode_pvrtc_device if pvrtc else ctx.encode_device)(group, params)
        except api.CfhipError as e:
            if e.code == api.E_UNSUPPORTED:
                return None
            raise
        return hosts, texels, pays

    def _adopt(self, payloads, format, type, alpha_type, color_mask):
        """convert()'s end state: the payloads in (mip, depth, face) order, the images freed"""
        it = iter(payloads)
        self._rdo_stats = None
        self._rdo_target = None
        self._textures = [[[next(it) for _ in dep] for dep in level] for level in self._images]
        self._images = [[[None]*len(dep) for dep in level] for level in self._images]
        self._format, self._type = format, type
        self._alpha, self._mask = Alpha(alpha_type), tuple(bool(m) for m in color_mask)

    def convert_rdo(self, format: Format, type: Type, quality: Quality = Quality.Normal,
                    alpha_type: Alpha = Alpha.Standard,
                    color_mask: Sequence[bool] = (True, True, True, True), rdo_lambda: float = 1.0,
                    max_sse_increase: Optional[int] = None, row_above: bool = False,
                    window_bytes: Optional[int] = None, target_ratio: Optional[float] = None) -> bool:
        """convert(), then the rate-distortion pass (Context.rdo_device) over the fresh payloads against the texels
        they were encoded from, in one visit to the device: every image is uploaded once, encoded from there,
        optimised in place, and only the final payloads and the statistics (rdo_stats()) come back.  The channels
        the pass measures are compare()'s: the colour mask's, without alpha when the alpha type is None.  Returns
        False wherever convert() does and for the formats the pass does not cover (api.rdo_supported); the texture
        is then left unconverted.  A lambda outside (0, 1024] raises api.CfhipError.  row_above and window_bytes are
        Context.rdo's: blocks may also copy from the block row above.
        target_ratio (None: the pass at rdo_lambda): the pass to a target (Context.rdo_target_device) -- the smallest
        lambda <= rdo_lambda whose payloads, all surfaces as one stream, are estimated at no more than target_ratio x
        the estimate of the plain ones.  Encoding still happens once, the search runs against the resident texels,
        rdo_stats() are the final pass's and rdo_target() returns the search's result."""
        import ctypes
        import torch
        if not self.images_complete() or not self.is_format_valid(format, type):
            return False
        format, type = Format(format), Type(type)
        if self._color_space == ColorSpace.sRGB and not self.has_native_srgb(format, type):
            return False
        if not api.rdo_supported(format, type):
            return False
        flat = [im for level in self._images for dep in level for im in dep]
        flat = [im.astype(np.float32) if im.dtype == np.float16 else im for im in flat]
        mask = [bool(m) for m in color_mask]
        if Alpha(alpha_type) == Alpha.None_ or not self.has_alpha(format):
            mask[3] = False
        params = api.make_params(format, type, quality, alpha_type, color_mask, self._color_space)
        ctx = self._context()
        resident = self._encode_resident(ctx, flat, format, type, params)
        if resident is None:
            return False
        hosts, texels, pays = resident
        size = ctypes.sizeof(api.RdoStats)
        stats = torch.empty(len(pays)*size, dtype=torch.uint8, device=pays[0].device)
        surfaces = [dict(blocks=p.data_ptr(), out=p.data_ptr(), out_capacity=p.numel(), pixels=t.data_ptr(),
                         pixel_type=int(api.pixel_type_of(h)), width=h.shape[1], height=h.shape[0],
                         row_pitch_bytes=h.strides[0]) for h, t, p in zip(hosts, texels, pays)]
        target = None
        if target_ratio is None:
            ctx.rdo_device(surfaces, format, type, rdo_lambda, stats.data_ptr(), max_sse_increase=max_sse_increase,
                           mask=mask, row_above=row_above, window_bytes=window_bytes)
        else:
            target = ctx.rdo_target_device(surfaces, format, type, target_ratio, rdo_lambda, stats.data_ptr(),
                                           max_sse_increase=max_sse_increase, mask=mask, row_above=row_above,
                                           window_bytes=window_bytes)
        raw = stats.cpu().numpy().tobytes()
        self._adopt([p.cpu().numpy() for p in pays], format, type, alpha_type, color_mask)
        self._rdo_target = target
        self._rdo_stats = [api.RdoStats.from_buffer_copy(raw[i*size:(i + 1)*size]).as_dict() for i in range(len(pays))]
        return True

    def rdo_stats(self):
        """The statistics of the last convert_rdo(), one dict per surface in (mip, depth, face) order; None before
        the first one."""
        return self._rdo_stats

    def rdo_target(self):
        """The result of the last convert_rdo(target_ratio=...): lambda16, reached, trials, est_bytes_plain,
        est_bytes_final; None when the last conversion had no target."""
        return self._rdo_target

    def packed_size(self):
        """The deflate-size estimate (Context.lz_size) of this converted texture's payloads, data() of every surface
        in (mip, depth, face) order as one stream; no container header is counted.  Any format.  None when the
        texture is not converted."""
        if not self._textures:
            return None
        return self._context().lz_size([p for _, _, _, p in self._flat()])

    def pack(self, indexed: bool = False, codec: str = "zlib"):
        """The zlib stream (Context.deflate) of this converted texture's payloads: data() of every surface in
        packed_size()'s order as one stream, for any format; zlib.decompress returns those bytes.  Its tokens are the
        ones packed_size() prices.  indexed=True: (the same stream, its index) from Context.deflate_indexed, what
        unpack() and Context.inflate_device read back on the GPU.  codec="lz4": one LZ4 frame (Context.lz4_encode)
        instead, which needs no index -- unpack() and Context.lz4_decode_device read it as it is, and so does the lz4
        tool; larger than the zlib stream (no entropy stage), worth it behind convert_rdo.  None when the texture is not
        converted."""
        if codec not in ("zlib", "lz4"):
            raise ValueError("codec must be 'zlib' or 'lz4'")
        if codec == "lz4" and indexed:
            raise ValueError("an LZ4 frame has no index: its blocks decode on their own")
        if not self._textures:
            return None
        ctx = self._context()
        payloads = [p for _, _, _, p in self._flat()]
        if codec == "lz4":
            out = ctx.lz4_encode(payloads)
            self._pack_result = ctx.lz4_encode_result()
            return out
        out = ctx.deflate_indexed(payloads) if indexed else ctx.deflate(payloads)
        self._pack_result = ctx.deflate_result()
        return out

    @staticmethod
    def unpack(like: "Texture", stream, index=None) -> Optional["Texture"]:
        """pack(indexed=True) undone on the GPU (Context.inflate): a converted texture with `like`'s layout, format,
        type, alpha type, colour mask and colour space whose surfaces are the inflated bytes -- one buffer, the
        surfaces views of it in storage order, as load() builds them.  With no index, a stream that begins with the LZ4
        magic is pack(codec="lz4")'s, or anyone's LZ4 frame of independent 64 KiB blocks, and goes through
        Context.lz4_decode.  None when `like` is not converted, and where the stream does not decode to exactly the
        bytes of like's payloads."""
        if not like._textures:
            return None
        sizes = [int(p.nbytes) for _, _, _, p in like._flat()]
        try:
            if index is None and bytes(stream[:4]) == api.LZ4_MAGIC:
                raw = like._context().lz4_decode(stream, sum(sizes))
            else:
                raw = like._context().inflate(stream, [] if index is None else index, sum(sizes))
        except (api.CfhipError, ValueError):
            return None
        t = Texture(device_id=like._device_id)
        if not t.initialize(like._dim, like._w, like._h, like._depth, like._mips, like._color_space):
            return None
        blob = np.frombuffer(raw, np.uint8)
        offs = np.cumsum([0] + sizes)
        it = iter(range(len(sizes)))
        t._textures = [[[blob[offs[i]:offs[i + 1]] for i in (next(it) for _ in dep)] for dep in level]
                       for level in like._textures]
        t._format, t._type, t._alpha, t._mask = like._format, like._type, like._alpha, like._mask
        return t

    def pack_result(self):
        """The cfhip_deflate_result (codec="lz4": the cfhip_lz4_result) of the last pack() as a dict; None before the
        first one."""
        return getattr(self, "_pack_result", None)

    def convert_and_compare(self, format: Format, type: Type, quality: Quality = Quality.Normal,
                            alpha_type: Alpha = Alpha.Standard,
                            color_mask: Sequence[bool] = (True, True, True, True), ssim: bool = True):
        """convert(), and the quality of the result against the images it was made from, in one visit to the
        device: every image is uploaded once, in the pixel type convert() hands to the encoder, encoded from there
        (Context.encode_device), the fresh payloads are measured against those same buffers, and only payloads and
        results come back.  Returns (results, pooled) -- exactly what compare(source) returns afterwards for an
        identical unconverted `source` -- or None wherever convert() returns False (the texture is then left
        unconverted).  The end state is convert()'s: the same payload bytes, the images freed.
        Block formats are measured by the batched entry (Context.compare_batch_device), standard formats and PVRTC
        by their per-surface device entries with compare()'s restrictions: PVRTC has no SSIM, so ssim must be
        False for it (ValueError, raised before any work).
        There is no strip pipeline here: the whole texture -- images, payloads and the compare's scratch -- is
        resident on the device during the call."""
        if not self.images_complete() or not self.is_format_valid(format, type):
            return None
        format, type = Format(format), Type(type)
        if self._color_space == ColorSpace.sRGB and not self.has_native_srgb(format, type):
            return None
        pvrtc = format in api.PVRTC_FORMATS
        flat = [im for level in self._images for dep in level for im in dep]
        if not (format == Format.BC6H or int(format) < int(Format.BC1_RGB)):
            flat = [im.astype(np.float32) if im.dtype == np.float16 else im for im in flat]
        if pvrtc:
            if any(im.shape[0] & (im.shape[0] - 1) or im.shape[1] & (im.shape[1] - 1) for im in flat):
                return None
            if ssim:
                raise ValueError("compare: PVRTC has no SSIM (pass ssim=False)")
        mask = [bool(m) for m in color_mask]
        if Alpha(alpha_type) == Alpha.None_ or not self.has_alpha(format):
            mask[3] = False
        if pvrtc and not any(mask):
            raise ValueError("compare: no channel compared")
        params = api.make_params(format, type, quality, alpha_type, color_mask, self._color_space)
        ctx = self._context()
        resident = self._encode_resident(ctx, flat, format, type, params)
        if resident is None:
            return None
        hosts, texels, pays = resident
        items = [(p, t, api.pixel_type_of(h), h.shape[1], h.shape[0]) for h, t, p in zip(hosts, texels, pays)]
        results = self._measure_device(ctx, format, type, items, mask, ssim)
        self._adopt([p.cpu().numpy() for p in pays], format, type, alpha_type, color_mask)
        if pvrtc:
            chans = [c for c in range(4) if mask[c]]
            return results, self._pooled_pvrtc(results, sum(h.shape[0]*h.shape[1] for h in hosts), chans)
        return results, self._pooled(results)

    def decode_image(self, *args) -> Optional[np.ndarray]:
        """decode_image([face,] mip=0, depth=0): the surface of this converted texture as the RGBAF image a
        cuttlefish::Image would hold, (h, w, 4) float32, for every format convert() accepts; None where data()
        returns None.  Standard formats through Context.unpack; block formats through Context.decode, normalised as
        cfhip_compare documents (RGBA8 v/255, SNorm max(v/127, -1), EAC v/2047 and max(v/1023, -1), halves ->
        float); PVRTC through Context.decode_pvrtc.  Channels the format does not store read 0, 0, 1.  The stored
        values are returned: no sRGB transfer."""
        payload = self.data(*args)
        if payload is None:
            return None
        _, mip, _ = self._face_args(args)
        w, h = self.width(mip), self.height(mip)
        ctx = self._context()
        if int(self._format) < int(Format.BC1_RGB):
            return ctx.unpack(payload, self._format, self._type, w, h)
        if self._format in api.PVRTC_FORMATS:
            raw, layout = ctx.decode_pvrtc(payload, self._format, w, h, self._type), api.Layout.RGBA8
        else:
            raw, _ = ctx.decode(payload, self._format, self._type, w, h)
            layout, _ = api.decoded_layout(self._format, self._type)
        out = np.zeros((h, w, 4), np.float32)
        out[..., 3] = 1.0
        n = raw.shape[2]
        if layout == api.Layout.RGBA16F:
            val = raw.astype(np.float32)
        else:
            div = {api.Layout.RGBA8: 255.0, api.Layout.R8: 255.0, api.Layout.RG8: 255.0, api.Layout.R8_SNorm: 127.0,
                   api.Layout.RG8_SNorm: 127.0, api.Layout.R16: 2047.0, api.Layout.RG16: 2047.0,
                   api.Layout.R16_SNorm: 1023.0, api.Layout.RG16_SNorm: 1023.0}[layout]
            val = np.maximum(raw.astype(np.float64)/div, -1.0).astype(np.float32)
        out[..., :n] = val
        return out

    def decoded_png(self, *args, bit_depth: int = 8) -> Optional[bytes]:
        """decoded_png([face,] mip=0, depth=0, bit_depth=8): the PNG file (RGBA, depth 8 or 16, an sRGB chunk for an
        sRGB texture) of one surface of this converted texture, decoded and written on the device: the payload goes up,
        Context.decode_batch_device (block formats), decode_pvrtc_device or unpack_device (standard formats) writes
        the texels, Context.png_encode_device reads them there and only the file comes back -- no host copy of texels.
        The file equals tests/png_ref.py on decode_image() of the surface.  Raises ValueError where decode_images()
        does (a format that does not decode to RGBA32F); None where data() returns None."""
        import torch
        if bit_depth not in (8, 16):
            raise ValueError("decoded_png: bit depth %r (8 or 16)" % (bit_depth,))
        payload = self.data(*args)
        if payload is None:
            return None
        _, mip, _ = self._face_args(args)
        w, h = self.width(mip), self.height(mip)
        ctx = self._context()
        dev = "cuda:%d" % self._device_id
        pvrtc = self._format in api.PVRTC_FORMATS
        block = int(self._format) >= int(Format.BC1_RGB) and not pvrtc
        pix, tb = (api.PixelType.RGBA8, 4) if pvrtc else (api.PixelType.RGBA32F, 16)
        if block and not api.decode_out_supported(self._format, self._type, pix):
            raise ValueError("decoded_png: %s / %s does not decode to %s" % (self._format.name, self._type.name, pix.name))
        blob = torch.from_numpy(np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1).copy()).to(dev)
        texels = torch.empty((h, w, tb), dtype=torch.uint8, device=dev)
        if block:
            ctx.decode_batch_device([dict(blocks=blob.data_ptr(), out=texels.data_ptr(), width=w, height=h,
                                          out_pitch_bytes=w*tb)], self._format, self._type, pix)
        elif pvrtc:
            ctx.decode_pvrtc_device(blob.data_ptr(), self._format, w, h, texels.data_ptr(), w*tb, self._type)
        else:
            ctx.unpack_device(blob.data_ptr(), self._format, self._type, w, h, texels.data_ptr(), w*tb)
        cap = api.png_bound(w, h, api.PNG_RGBA, bit_depth, self._color_space)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        res = torch.empty(15, dtype=torch.int64, device=dev)               # one cfhip_png_result
        ctx.png_encode_device(texels.data_ptr(), pix, w*tb, w, h, out.data_ptr(), cap, res.data_ptr(),
                              color_type=api.PNG_RGBA, bit_depth=bit_depth, color_space=self._color_space)
        return out[:int(res[0].item())].cpu().numpy().tobytes()

    def _flat(self):
        """[(mip, depth, face, payload)] in storage order"""
        return [(m, d, f, p) for m, level in enumerate(self._textures) for d, dep in enumerate(level)
                for f, p in enumerate(dep)]

    def decode_images(self, pixel=api.PixelType.RGBA32F):
        """Every surface of this converted texture as [mip][depth][face] arrays of `pixel` ((h, w, 4)); RGBA32F
        equals decode_image() of each surface bit for bit.  Block formats decode in ONE batched launch
        (Context.decode_batch); standard formats and PVRTC go through their per-surface entries, which offer
        RGBA32F and RGBA8 respectively (PVRTC as RGBA32F is v / 255 of those bytes).  Raises ValueError for a pixel
        type the format does not offer; None when the texture is not converted."""
        if not self._textures:
            return None
        pixel = api.PixelType(pixel)
        flat = self._flat()
        ctx = self._context()
        if int(self._format) >= int(Format.BC1_RGB) and self._format not in api.PVRTC_FORMATS:
            if not api.decode_out_supported(self._format, self._type, pixel):
                raise ValueError("decode_images: %s / %s does not decode to %s" %
                                 (self._format.name, self._type.name, pixel.name))
            outs, _ = ctx.decode_batch([p for _, _, _, p in flat], self._format, self._type,
                                       [(self.width(m), self.height(m)) for m, _, _, _ in flat], pixel)
        elif self._format in api.PVRTC_FORMATS:
            if pixel == api.PixelType.RGBA16F:
                raise ValueError("decode_images: PVRTC decodes to RGBA8 or RGBA32F")
            outs = [ctx.decode_pvrtc(p, self._format, self.width(m), self.height(m), self._type) for m, _, _, p in flat]
            if pixel == api.PixelType.RGBA32F:
                outs = [(o.astype(np.float64)/255.0).astype(np.float32) for o in outs]
        else:
            if pixel != api.PixelType.RGBA32F:
                raise ValueError("decode_images: standard formats unpack to RGBA32F")
            outs = [ctx.unpack(p, self._format, self._type, self.width(m), self.height(m)) for m, _, _, p in flat]
        it = iter(outs)
        return [[[next(it) for _ in dep] for dep in level] for level in self._textures]

    def transcode(self, format, type, quality: Quality = Quality.Normal, alpha_type: Optional[Alpha] = None,
                  color_mask: Sequence[bool] = (True, True, True, True), regenerate_mips: bool = False,
                  filter=api.ResizeFilter.CatmullRom, measure: bool = False, ssim: bool = True):
        """A new converted texture of the same shape in another (format, type), made on the device: the payloads
        are uploaded, decoded into device buffers (one batched launch for block formats), encoded from there with
        cfhip_encode_device / cfhip_pvrtc_encode_device and only the new payloads come back.  regenerate_mips:
        only level 0 is decoded and the other levels (as many as this texture has) come from
        cfhip_generate_mips_array_device with `filter`.  The colour space and, unless given, the alpha type carry
        over.  None where convert() would return False, and when this texture is not converted.
        The result is byte-identical to an unconverted Texture built from decode_image() of every surface (of
        level 0, then generate_mipmaps(filter, mip_levels=mip_level_count()), when regenerating) and convert()
        with the same arguments.  3-D textures with regenerate_mips take that host route itself.
        measure=True: returns (texture, results, pooled) instead, results and pooled as compare() returns them, the
        reference being the intermediate the encoder read -- the decoded RGBA8 or RGBA32F texels and the
        regenerated RGBA32F levels -- still on the device: each new payload is measured as Context.compare measures
        it against decode_images(pixel) of this texture (or against the regenerated level), with the mask compare()
        uses, one compare call per pixel type as the encode makes.  The two host routes measure with compare() on
        the host.  ssim as in compare(): a PVRTC target needs ssim=False (ValueError, raised before any work)."""
        import torch
        if not self._textures or not self.is_format_valid(format, type):
            return None
        format, type = Format(format), Type(type)
        if self._color_space == ColorSpace.sRGB and not self.has_native_srgb(format, type):
            return None
        alpha_type = self._alpha if alpha_type is None else Alpha(alpha_type)
        pvrtc_out = format in api.PVRTC_FORMATS
        if pvrtc_out and any(v & (v - 1) for m in range(self._mips) for v in (self.width(m), self.height(m))):
            return None
        if measure and pvrtc_out and ssim:
            raise ValueError("compare: PVRTC has no SSIM (pass ssim=False)")
        out = Texture(self._dim, self._w, self._h, self._depth, self._mips, self._color_space,
                      device_id=self._device_id)
        out._ctx = self._ctx
        src_block = int(self._format) >= int(Format.BC1_RGB) and self._format not in api.PVRTC_FORMATS
        src_pvrtc = self._format in api.PVRTC_FORMATS
        # the intermediate: RGBA8 where the source offers it and the target quantises its source to 8 bits (the
        # encoder's round(clamp(f) * 255) of (float)(v / 255.0) is v again); RGBA32F otherwise
        to8 = (type == Type.UNorm and int(format) >= int(Format.BC1_RGB) and
               format not in (Format.EAC_R11, Format.EAC_R11G11))        # EAC keeps more than 8 bits of a float
        if (regenerate_mips and self._dim == Dimension.Dim3D) or (src_pvrtc and not to8):
            # the defined route itself, through the host: 3-D chains (generated along the depth too) and PVRTC
            # sources, which decode to RGBA8 only, into targets that read floats
            for m, d, f, _ in self._flat():
                if m == 0 or not regenerate_mips:
                    args = (CubeFace(f), m, d) if self._faces == 6 else (m, d)
                    out._images[m][d][f] = self.decode_image(*args)
            if regenerate_mips and not out.generate_mipmaps(filter, mip_levels=self._mips):
                return None
            if not measure:
                return out if out.convert(format, type, quality, alpha_type, color_mask) else None
            source = Texture(self._dim, self._w, self._h, self._depth, self._mips, self._color_space,
                             device_id=self._device_id)
            source._ctx = self._ctx
            source._images = [[list(dep) for dep in level] for level in out._images]
            if not out.convert(format, type, quality, alpha_type, color_mask):
                return None
            return (out,) + tuple(out.compare(source, ssim=ssim))
        ctx = self._context()
        dev = "cuda:%d" % self._device_id
        flat = [s for s in self._flat() if not regenerate_mips or s[0] == 0]
        if src_pvrtc or (src_block and to8 and api.decode_out_supported(self._format, self._type, api.PixelType.RGBA8)):
            pix, tb = api.PixelType.RGBA8, 4
        else:
            pix, tb = api.PixelType.RGBA32F, 16
        blob = torch.from_numpy(np.concatenate([np.ascontiguousarray(p, dtype=np.uint8).reshape(-1)
                                                for _, _, _, p in flat])).to(dev)
        offs, o = [], 0
        for _, _, _, p in flat:
            offs.append(o)
            o += int(p.nbytes)
        texels = [torch.empty((self.height(m), self.width(m), tb), dtype=torch.uint8, device=dev) for m, _, _, _ in flat]
        if src_block:
            ctx.decode_batch_device([dict(blocks=blob.data_ptr() + off, out=t.data_ptr(), width=self.width(m),
                                          height=self.height(m), out_pitch_bytes=self.width(m)*tb)
                                     for (m, _, _, _), off, t in zip(flat, offs, texels)],
                                    self._format, self._type, pix)
        else:
            # per-surface entries; a payload inside the blob may sit at any offset, PVRTC wants 4-byte alignment
            # (its payloads are multiples of 8 bytes, so the offsets are)
            for (m, _, _, _), off, t in zip(flat, offs, texels):
                if src_pvrtc:
                    ctx.decode_pvrtc_device(blob.data_ptr() + off, self._format, self.width(m), self.height(m),
                                            t.data_ptr(), self.width(m)*4, self._type)
                else:
                    ctx.unpack_device(blob.data_ptr() + off, self._format, self._type, self.width(m), self.height(m),
                                      t.data_ptr(), self.width(m)*16)
        # sources of the encode: (mip, depth, face, tensor, pixel type)
        srcs = [(m, d, f, t, pix) for (m, d, f, _), t in zip(flat, texels)]
        if regenerate_mips and self._mips > 1:
            gen = [[torch.empty((self.height(m), self.width(m), 4), dtype=torch.float32, device=dev)
                    for m in range(1, self._mips)] for _ in srcs]
            ctx.generate_mips_array_device([t.data_ptr() for _, _, _, t, _ in srcs], pix, self._w, self._h,
                                           self._w*tb, [[g.data_ptr() for g in chain] for chain in gen],
                                           color_space=self._color_space, filter=int(api.ResizeFilter(filter)))
            for (_, d, f, _, _), chain in zip(list(srcs), gen):
                srcs += [(m, d, f, g, api.PixelType.RGBA32F) for m, g in enumerate(chain, start=1)]
        params = api.make_params(format, type, quality, alpha_type, color_mask, self._color_space)
        size = (api.pvrtc_payload_size if pvrtc_out else api.payload_size)
        pays = [torch.empty(size(format, type, self.width(m), self.height(m)), dtype=torch.uint8, device=dev)
                for m, _, _, _, _ in srcs]
        surfaces = [dict(pixels=t.data_ptr(), pixel_type=int(pt), width=self.width(m), height=self.height(m),
                         row_pitch_bytes=self.width(m)*(4 if pt == api.PixelType.RGBA8 else 16), out=p.data_ptr(),
                         out_capacity=p.numel()) for (m, _, _, t, pt), p in zip(srcs, pays)]
        try:
            # one call per pixel type: level 0 may be RGBA8 where the regenerated levels are RGBA32F
            for pt in sorted({s["pixel_type"] for s in surfaces}):
                group = [s for s in surfaces if s["pixel_type"] == pt]
                (ctx.encode_pvrtc_device if pvrtc_out else ctx.encode_device)(group, params)
        except api.CfhipError as e:
            if e.code == api.E_UNSUPPORTED:
                return None
            raise
        measured = None
        if measure:
            mask = [bool(c) for c in color_mask]
            if alpha_type == Alpha.None_ or not self.has_alpha(format):
                mask[3] = False
            # storage order, as compare() lists its results
            order = sorted(range(len(srcs)), key=lambda i: srcs[i][:3])
            measured = self._measure_device(ctx, format, type, [(pays[i], srcs[i][3], srcs[i][4], self.width(srcs[i][0]),
                                                                 self.height(srcs[i][0])) for i in order], mask, ssim)
        host = {(m, d, f): p.cpu().numpy() for (m, d, f, _, _), p in zip(srcs, pays)}
        out._textures = [[[host[(m, d, f)] for f in range(self._faces)] for d in range(self.depth(m))]
                         for m in range(self._mips)]
        out._images = [[[None]*self._faces for _ in range(self.depth(m))] for m in range(self._mips)]
        out._format, out._type = format, type
        out._alpha, out._mask = alpha_type, tuple(bool(c) for c in color_mask)
        if measure:
            if pvrtc_out:
                chans = [c for c in range(4) if mask[c]]
                if not chans:
                    raise ValueError("compare: no channel compared")
                texels = sum(self.width(m)*self.height(m) for m, _, _, _, _ in srcs)
                return out, measured, self._pooled_pvrtc(measured, texels, chans)
            return out, measured, self._pooled(measured)
        return out

    def _compare_pvrtc(self, ctx, source, mask, ssim):
        """compare() for PVRTC1 4 bpp: PSNR from the fused decode + SSE (cfhip_pvrtc_decode_sse) against the
        source quantised to RGBA8 as the encoder quantises it.  No SSIM and no error map for PVRTC.  Returns
        (per surface: [sse r, g, b, a], the pooled PSNR over the compared channels)."""
        if ssim:
            raise ValueError("compare: PVRTC has no SSIM (pass ssim=False)")
        chans = [c for c in range(4) if mask[c]]
        if not chans:
            raise ValueError("compare: no channel compared")
        results = []
        for m, level in enumerate(self._textures):
            for d, dep in enumerate(level):
                for f, payload in enumerate(dep):
                    ref = _rgba8_of(source._images[m][d][f])
                    results.append(ctx.decode_pvrtc_sse(payload, ref, self._format, self._type))
        n = sum(int(np.prod(source._images[m][d][f].shape[:2]))
                for m, level in enumerate(self._textures) for d, dep in enumerate(level) for f in range(len(dep)))
        return results, self._pooled_pvrtc(results, n, chans)

    # ---- saving (Texture.cpp:1636-1685) --------------------------------------------------------
    def _layout(self) -> containers.TextureLayout:
        dim = {Dimension.Dim1D: "1d", Dimension.Dim2D: "2d", Dimension.Dim3D: "3d", Dimension.Cube: "cube"}[self._dim]
        surfaces = [[[f.tobytes() for f in dep] for dep in level] for level in self._textures]
        return containers.TextureLayout(self._format, self._type, self._w, self._h, surfaces, dimension=dim,
                                        depth=self._depth)

    def save_bytes(self, file_type: FileType) -> Tuple[SaveResult, bytes]:
        """Texture::save(std::vector<uint8_t>&, fileType)."""
        if not self.converted():
            return SaveResult.Invalid, b""
        try:
            file_type = FileType(file_type)
        except ValueError:
            return SaveResult.UnknownFormat, b""
        buf = io.BytesIO()
        try:
            if file_type == FileType.DDS:
                containers.write_dds_texture(buf, self._layout(), self._color_space, self._alpha)
            elif file_type == FileType.KTX:
                containers.write_ktx_texture(buf, self._layout(), self._color_space)
            elif file_type == FileType.PVR:
                if not self.is_format_valid(self._format, self._type, FileType.PVR):
                    return SaveResult.Unsupported, b""
                containers.write_pvr_texture(buf, self._layout(), self._color_space, self._alpha)
            else:
                return SaveResult.UnknownFormat, b""
        except ValueError:
            return SaveResult.Unsupported, b""      # no DXGI / GL / PVR form of this (format, type)
        return SaveResult.Success, buf.getvalue()

    def save(self, file_name: Optional[str], file_type: FileType = FileType.Auto) -> SaveResult:
        """Texture::save(fileName, fileType = Auto)."""
        if not self.converted() or not file_name:
            return SaveResult.Invalid
        if FileType(file_type) == FileType.Auto:
            file_type = self.file_type(file_name)
        try:
            stream = open(file_name, "wb")
        except OSError:
            return SaveResult.WriteError
        with stream:
            result, payload = self.save_bytes(file_type)
            if result == SaveResult.Success:
                try:
                    stream.write(payload)
                except OSError:
                    return SaveResult.WriteError
        return result
