"""cuttlefish::Image's pixel operations (lib/src/Image.cpp:1513-1882) on the GPU, and the cuttlefish tool's per-image
pipeline (tool/main.cpp:147-277, loadAndProcessImage) from a loaded image to the array Texture.set_image takes.

Pixels are (h, w, 4) numpy arrays, row 0 at the top (Image::getPixel(x, 0)), uint8 / float16 / float32 read as the
reference's RGBAF image (uint8 as v/255).  Every op runs in csrc/image_ops.hip (cfhip_image_ops_device) and
returns RGBA32F; there is no CPU path.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import api
from .api import Channel, ColorSpace, ImageOp, NormalOptions, ResizeFilter, RotateAngle, Type
from .texture import ImageFormat, Texture

_contexts: Dict[int, api.Context] = {}


def _context(device_id: int) -> api.Context:
    if device_id not in _contexts:
        _contexts[device_id] = api.Context(device_id)
    return _contexts[device_id]


def _pixels(image) -> np.ndarray:
    a = np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("expected an (h, w, 4) image, got shape %r" % (a.shape,))
    if a.dtype not in (np.uint8, np.float16, np.float32):
        a = a.astype(np.float32)
    return a


def _quarter(angle) -> bool:
    return RotateAngle(angle) not in (RotateAngle.CW180, RotateAngle.CCW180)


class _Device:
    """The device calls of process_image and Image: upload, one fused ops pass, one resize, download.  Buffers
    are torch tensors (plumbing only); a buffer is (tensor, pixel type, width, height, row pitch in bytes)."""

    def __init__(self, device_id: int = 0):
        self.ctx = _context(device_id)
        self.device = "cuda:%d" % device_id

    def upload(self, pixels: np.ndarray):
        import torch
        host = np.ascontiguousarray(pixels)
        t = torch.from_numpy(host).to(self.device)
        return (t, api.pixel_type_of(host), host.shape[1], host.shape[0], host.strides[0])

    def ops(self, buf, ops: api.ImageOps):
        import torch
        t, pt, w, h, pitch = buf
        rw, rh = (h, w) if (ops.ops & ImageOp.Rotate) and _quarter(ops.rotate) else (w, h)
        dst = torch.empty((rh, rw, 4), dtype=torch.float32, device=t.device)
        self.ctx.image_ops_device(t.data_ptr(), pt, w, h, pitch, ops, dst.data_ptr(), rw * 16)
        return (dst, api.PixelType.RGBA32F, rw, rh, rw * 16)

    def resize(self, buf, width: int, height: int, color_space, filter):
        import torch
        t, pt, w, h, pitch = buf
        dst = torch.empty((height, width, 4), dtype=torch.float32, device=t.device)
        self.ctx.resize_device(t.data_ptr(), pt, w, h, pitch, dst.data_ptr(), width, height,
                               color_space=color_space, filter=int(filter))
        return (dst, api.PixelType.RGBA32F, width, height, width * 16)

    def download(self, buf) -> np.ndarray:
        return buf[0].cpu().numpy()

    def bleed(self, buf, threshold: float = 0.0, wrap=False, max_distance: int = 0):
        """Alpha bleeding of a buffer in place (cfhip_alpha_bleed_array_device) -> the buffer"""
        t, pt, w, h, pitch = buf
        self.ctx.alpha_bleed_device([t.data_ptr()], pt, w, h, pitch, threshold, wrap, max_distance)
        return buf

    def sdf(self, src, dst, spread: int, threshold: float = 0.5, wrap=False, channels="a"):
        """The signed distance field of src's alpha (cfhip_alpha_sdf_array_device) into the named channels of dst, a
        buffer 1, 2, 4, 8 or 16 times smaller per side (src itself: in place) -> dst"""
        t, pt, w, h, pitch = src
        dt, dpt, dw, dh, dpitch = dst
        self.ctx.alpha_sdf_device([t.data_ptr()], pt, w, h, pitch, [dt.data_ptr()], dpt, dpitch, spread, w // dw,
                                  threshold, wrap, channels)
        return dst

    def ao(self, src, dst, radius: int, **kw):
        """The ambient occlusion of src's height channel (cfhip_height_ao_array_device) into the named channels of dst,
        a buffer of the same size (src itself: in place) -> dst.  kw: Context.height_ao_device's keywords."""
        t, pt, w, h, pitch = src
        dt, dpt, dw, dh, dpitch = dst
        self.ctx.height_ao_device([t.data_ptr()], pt, w, h, pitch, [dt.data_ptr()], dpt, dpitch, radius=radius, **kw)
        return dst

    def png(self, buf, color_type: int, bit_depth: int, color_space) -> bytes:
        """The PNG file of a buffer (cfhip_png_encode_device): only the file's bytes come back."""
        import torch
        t, pt, w, h, pitch = buf
        cap = api.png_bound(w, h, color_type, bit_depth, color_space)
        out = torch.empty(cap, dtype=torch.uint8, device=t.device)
        res = torch.empty(15, dtype=torch.int64, device=t.device)          # one cfhip_png_result
        self.ctx.png_encode_device(t.data_ptr(), pt, pitch, w, h, out.data_ptr(), cap, res.data_ptr(),
                                   color_type=color_type, bit_depth=bit_depth, color_space=color_space)
        return out[:int(res[0].item())].cpu().numpy().tobytes()


class Image:
    """A numpy-backed mirror of cuttlefish::Image's pixel methods, under the reference's names.  Each op runs on
    the GPU and leaves the pixels as an RGBA32F host array.  An RGBF image (what create_normal_map returns) keeps
    alpha at 1: swizzle drops the alpha it would write and pre_multiply_alpha does nothing."""

    def __init__(self, pixels, color_space: ColorSpace = ColorSpace.Linear, rgbf: bool = False, device_id: int = 0):
        self.pixels = _pixels(pixels)
        self.color_space = ColorSpace(color_space)
        self.rgbf = bool(rgbf)
        self.device_id = device_id
        self._last = None       # (the device buffer the last op wrote, the host array downloaded from it)

    @property
    def width(self) -> int:
        return self.pixels.shape[1]

    @property
    def height(self) -> int:
        return self.pixels.shape[0]

    def _run(self, ops: int, **fields) -> np.ndarray:
        d = _Device(self.device_id)
        desc = api.make_image_ops(ops, self.color_space, rgbf=self.rgbf, **fields)
        buf = d.ops(d.upload(self.pixels), desc)
        out = d.download(buf)
        self._last = (buf, out)
        return out

    def _derived(self, pixels, color_space=None, rgbf=None) -> "Image":
        img = Image(pixels, self.color_space if color_space is None else color_space,
                    self.rgbf if rgbf is None else rgbf, self.device_id)
        if self._last is not None and self._last[1] is img.pixels:
            img._last, self._last = self._last, None          # the buffer belongs to the new image
        return img

    def save_bytes(self, color_type: Optional[int] = None, bit_depth: int = 8) -> bytes:
        """The PNG file Image::save writes for the .png extension, made on the GPU (Context.png_encode_device): colour
        type 0 (grey: the red channel), 2, 4 or 6 -- None: RGBA, or RGB for an RGBF image -- at depth 8 or 16, with an
        sRGB chunk when the image's colour space is sRGB.  The pixels go from the device buffer the last op left them
        in while `pixels` is still the array that op returned (assigning another array uploads that one; an array
        edited in place is not noticed); only the file's bytes come back."""
        if color_type is None:
            color_type = api.PNG_RGB if self.rgbf else api.PNG_RGBA
        if color_type not in (api.PNG_GREY, api.PNG_RGB, api.PNG_GREY_ALPHA, api.PNG_RGBA):
            raise ValueError("save: colour type %r (0, 2, 4 or 6)" % (color_type,))
        if bit_depth not in (8, 16):
            raise ValueError("save: bit depth %r (8 or 16)" % (bit_depth,))
        d = _Device(self.device_id)
        if self._last is not None and self._last[1] is self.pixels:
            buf = self._last[0]
        else:
            buf = d.upload(self.pixels)
        return d.png(buf, int(color_type), int(bit_depth), self.color_space)

    def save(self, file_name: str, color_type: Optional[int] = None, bit_depth: int = 8) -> bool:
        """Image::save: writes save_bytes() to file_name when its extension is .png; any other extension returns
        False and writes nothing."""
        import os
        if os.path.splitext(str(file_name))[1].lower() != ".png":
            return False
        data = self.save_bytes(color_type, bit_depth)
        with open(file_name, "wb") as f:
            f.write(data)
        return True

    def flip_horizontal(self) -> bool:
        self.pixels = self._run(ImageOp.FlipX)
        return True

    def flip_vertical(self) -> bool:
        self.pixels = self._run(ImageOp.FlipY)
        return True

    def rotate(self, angle: RotateAngle) -> "Image":
        """A new image; width and height swap for 90 and 270 degrees."""
        return self._derived(self._run(ImageOp.Rotate, rotate=RotateAngle(angle)))

    def pre_multiply_alpha(self) -> bool:
        self.pixels = self._run(ImageOp.PreMultiply)
        return True

    def bleed_alpha(self, threshold: float = 0.0, wrap=False, max_distance: int = 0) -> bool:
        """Alpha bleeding (Context.alpha_bleed_device): every texel with alpha <= threshold takes the colour of the
        nearest texel with alpha > threshold, bit for bit; alpha and the pixel type stay.  The remedy of straight alpha
        for fringes in mips and for block endpoints spent on hidden colour -- the alternative to pre_multiply_alpha,
        not a companion.  wrap: a bool or (x, y) for tiling images; max_distance: texels, 0 = unlimited.  False for
        an RGBF image: it has no alpha."""
        if self.rgbf:
            return False
        d = _Device(self.device_id)
        buf = d.bleed(d.upload(self.pixels), threshold, wrap, max_distance)
        self.pixels = d.download(buf)
        self._last = (buf, self.pixels)
        return True

    def distance_field(self, spread: int, scale: int = 1, threshold: float = 0.5, wrap=False,
                       channels="a") -> Optional["Image"]:
        """A signed distance field from this image's alpha (Context.alpha_sdf_device) as a new image of
        width/scale x height/scale: texels with alpha > threshold are inside, and the named channels take the Euclidean
        distance to the silhouette, exact up to `spread` source texels -- 0.5 on the edge, 0 a spread outside, 1 a spread
        inside -- averaged over scale x scale texels.  Sampled bilinearly and tested against 0.5, it magnifies to a clean
        edge where a small alpha mask goes blocky.  The other channels are this image's at scale 1 (the pixel type
        stays), and at scale 2, 4, 8 or 16 those of resize(width/scale, height/scale, Box), an RGBA32F image.  wrap: a
        bool or (x, y) for tiling images.  None for an RGBF image: it has no alpha."""
        if self.rgbf:
            return None
        api.make_sdf_params(spread, scale, threshold, wrap, channels)
        if self.width % scale or self.height % scale:
            raise ValueError("%dx%d is not a multiple of the scale %d" % (self.width, self.height, scale))
        d = _Device(self.device_id)
        src = d.upload(self.pixels)
        if scale == 1:
            dst = (src[0].clone(),) + src[1:]
        else:
            dst = d.resize(src, self.width // scale, self.height // scale, self.color_space, ResizeFilter.Box)
        buf = d.sdf(src, dst, spread, threshold, wrap, channels)
        out = d.download(buf)
        self._last = (buf, out)
        return self._derived(out)

    def ambient_occlusion(self, radius: int, height: float = 1.0, directions: int = 16, channel="r", channels="r",
                          strength: float = 1.0, bias: float = 0.0, uniform: bool = False, falloff: bool = False,
                          wrap=False) -> Optional["Image"]:
        """The occlusion this image's height field casts on itself (Context.height_ao_device) as a new image of the
        same size and pixel type: `channel` holds the heights, `height` texels per stored unit -- the meaning
        create_normal_map's height has, so one value gives consistent normals and occlusion -- and the named
        `channels` take the share of the sky the horizons within `radius` texels leave open, 1 on a flat surface.  The
        other channels are this image's.  directions: 8, 16 or 32; strength, bias, uniform, falloff:
        api.make_height_ao_params; wrap: a bool or (x, y) for tiling images.  None for an RGBF image, as
        distance_field answers one."""
        if self.rgbf:
            return None
        kw = dict(height_scale=height, directions=directions, channel=channel, channels=channels, strength=strength,
                  bias=bias, uniform=uniform, falloff=falloff, wrap=wrap)
        api.make_height_ao_params(radius, **kw)
        d = _Device(self.device_id)
        import torch
        src = d.upload(self.pixels)
        dst = (src[0].clone(),) + src[1:]
        torch.cuda.current_stream(src[0].device).synchronize()     # the context's stream does not wait for the copy
        buf = d.ao(src, dst, radius, **kw)
        out = d.download(buf)
        self._last = (buf, out)
        return self._derived(out)

    def change_color_space(self, color_space: ColorSpace) -> bool:
        self.pixels = self._run(ImageOp.ColorSpace, dst_color_space=ColorSpace(color_space))
        self.color_space = ColorSpace(color_space)
        return True

    def grayscale(self) -> bool:
        self.pixels = self._run(ImageOp.Grayscale)
        return True

    def swizzle(self, red: Channel, green: Channel, blue: Channel, alpha: Channel) -> bool:
        self.pixels = self._run(ImageOp.Swizzle, swizzle=(Channel(red), Channel(green), Channel(blue),
                                                          Channel(alpha)))
        return True

    def create_normal_map(self, options: NormalOptions = NormalOptions.Default, height: float = 1.0) -> "Image":
        """A new RGBF image of the same size, from the red channel."""
        return self._derived(self._run(ImageOp.NormalMap, normal_options=NormalOptions(options),
                                       normal_height=height), rgbf=True)

    def resize(self, width: int, height: int, filter: ResizeFilter = ResizeFilter.CatmullRom) -> "Image":
        """Image::resize through cfhip_resize_device, in linear space for an sRGB image; equal sizes copy."""
        d = _Device(self.device_id)
        buf = d.resize(d.upload(self.pixels), width, height, self.color_space, filter)
        out = d.download(buf)
        self._last = (buf, out)
        return self._derived(out)


_SIGNED = (Type.SNorm, Type.Int, Type.Float)      # isSigned (tool/main.cpp:63-75)
_AO_KEYS = ("radius", "height", "directions", "channel", "channels", "strength", "bias", "uniform", "falloff", "wrap")


def plan_process_image(width: int, height: int, src_width: int, src_height: int, image_color_space,
                       texture_color_space, mip_level: int = 0, type=Type.UNorm, rotate=None,
                       grayscale: bool = False, normal_map=None, flip_x: bool = False, flip_y: bool = False,
                       swizzle=None, premultiply: bool = False, bleed: Optional[dict] = None,
                       sdf: Optional[dict] = None, ao: Optional[dict] = None):
    """The device steps of process_image, in order: ("ops", ImageOps) and ("resize", width, height, colour space).
    At most three ops steps: before the first resize, between the resizes, after the last.  bleed = dict(threshold=,
    wrap=, max_distance=) (any of them; Image.bleed_alpha's defaults) adds one ("bleed", threshold, wrap, max_distance)
    step directly before the first resize -- after the ops pass in front of it, so that the filter's taps find the bled
    colour -- or after the last ops step when nothing is resized; None adds nothing.  With premultiply it raises
    ValueError: bleeding is the remedy of straight alpha.
    sdf = dict(spread=, threshold=, wrap=, channels=) (spread required; Image.distance_field's defaults) adds two steps:
    ("sdf_class",) where a bleed step would go -- the buffer whose alpha gives the classes, after the bleed if there is
    one -- and ("sdf", spread, scale, threshold, wrap, channels) directly after the resize that follows it, which writes
    the field over the resized image's channels before any later ops step moves texels; nothing resized: scale 1, in
    place.  The scale is the size before that resize divided by the size after it: ValueError unless it is 1, 2, 4, 8
    or 16 on both axes, and with premultiply (the field replaces an alpha that is no longer coverage).  None adds
    nothing.
    ao = dict(radius=, height=, directions=, channel=, channels=, strength=, bias=, uniform=, falloff=, wrap=) (radius
    required; Image.ambient_occlusion's defaults) adds one ("ao", radius, keywords of Context.height_ao_device) step
    where a bleed step would go, after the bleed if there is one: the occlusion of the height channel, in place.  With
    normal_map it raises ValueError: the height is gone after that op."""
    ao_step = None
    if ao is not None:
        if normal_map is not None:
            raise ValueError("ao and normal_map exclude each other: the height is gone after the normal-map op")
        unknown = set(ao) - set(_AO_KEYS)
        if unknown or "radius" not in ao:
            raise ValueError("ao: radius and any of %s; not %r" % (", ".join(_AO_KEYS[1:]), sorted(ao)))
        kw = {("height_scale" if k == "height" else k): v for k, v in ao.items() if k != "radius"}
        api.make_height_ao_params(ao["radius"], **kw)
        ao_step = ("ao", ao["radius"], kw)
    sdf_step = None
    if sdf is not None:
        if premultiply:
            raise ValueError("sdf and premultiply exclude each other: a distance in alpha is not a coverage to multiply by")
        unknown = set(sdf) - {"spread", "threshold", "wrap", "channels"}
        if unknown or "spread" not in sdf:
            raise ValueError("sdf: spread and any of threshold, wrap, channels; not %r" % (sorted(sdf),))
        sdf_step = (sdf["spread"], float(sdf.get("threshold", 0.5)), api.wrap_axes(sdf.get("wrap", False)),
                    sdf.get("channels", "a"))
    bleed_step = None
    if bleed is not None:
        if premultiply:
            raise ValueError("bleed and premultiply exclude each other: alpha bleeding is for straight alpha")
        unknown = set(bleed) - {"threshold", "wrap", "max_distance"}
        if unknown:
            raise ValueError("bleed: unknown keys %r" % (sorted(unknown),))
        bleed_step = ("bleed", float(bleed.get("threshold", 0.0)), api.wrap_axes(bleed.get("wrap", False)),
                      int(bleed.get("max_distance", 0)))
    steps = []
    cs = ColorSpace(image_color_space)
    tcs = ColorSpace(texture_color_space)
    this_w, this_h = max(width >> mip_level, 1), max(height >> mip_level, 1)
    normal = normal_map is not None
    # with a normal map at a mip level the map is made at the full target size, then resized (main.cpp:181-190)
    normal_w, normal_h = (width, height) if normal else (this_w, this_h)
    group = {"ops": 0, "src": cs}
    fields = {}

    def close(final=False):
        # a group before a resize runs only when it has ops (the resize reads any pixel type); the last one also
        # when nothing else ran (the result is RGBA32F), and after a normal map always: a resize can leave alpha
        # a rounding step away from 1, the reference's RGBF image has none
        nonlocal group, fields
        if group["ops"] or (final and (normal or not steps)):
            steps.append(("ops", api.make_image_ops(group["ops"], group["src"], dst_color_space=tcs,
                                                    rgbf=final and normal, **fields)))
        group, fields = {"ops": 0, "src": cs}, {}

    if tcs != cs:
        group["ops"] |= ImageOp.ColorSpace
        cs = tcs
    if (normal_w, normal_h) != (src_width, src_height):
        close()
        steps.append(("resize", normal_w, normal_h, cs))
    if rotate is not None:
        group["ops"] |= ImageOp.Rotate
        fields["rotate"] = RotateAngle(rotate)
    if grayscale:
        group["ops"] |= ImageOp.Grayscale
    if normal:
        options, nheight = normal_map
        options = NormalOptions(options)
        if Type(type) in _SIGNED:
            options |= NormalOptions.KeepSign
        group["ops"] |= ImageOp.NormalMap
        fields["normal_options"] = options
        fields["normal_height"] = float(nheight)
        if (normal_w, normal_h) != (this_w, this_h):
            close()
            steps.append(("resize", this_w, this_h, cs))
    if flip_x:
        group["ops"] |= ImageOp.FlipX
    if flip_y:
        group["ops"] |= ImageOp.FlipY
    if swizzle is not None:
        group["ops"] |= ImageOp.Swizzle
        fields["swizzle"] = tuple(Channel(c) for c in swizzle)
    if premultiply:
        group["ops"] |= ImageOp.PreMultiply
    close(final=True)
    if bleed_step is not None:
        first = next((i for i, st in enumerate(steps) if st[0] == "resize"), len(steps))
        steps.insert(first, bleed_step)
    if ao_step is not None:
        first = next((i for i, st in enumerate(steps) if st[0] == "resize"), len(steps))
        steps.insert(first, ao_step)
    if sdf_step is not None:
        first = next((i for i, st in enumerate(steps) if st[0] == "resize"), len(steps))
        before, after = (src_width, src_height), (steps[first][1:3] if first < len(steps) else (src_width, src_height))
        scale = before[0] // after[0]
        if scale not in api.SDF_SCALES or (after[0]*scale, after[1]*scale) != before:
            raise ValueError("sdf: %dx%d to %dx%d is not a scale of 1, 2, 4, 8 or 16 on both axes" % (before + tuple(after)))
        api.make_sdf_params(sdf_step[0], scale, sdf_step[1], sdf_step[2], sdf_step[3])
        steps.insert(first, ("sdf_class",))
        steps.insert(min(first + 2, len(steps)), ("sdf", sdf_step[0], scale) + sdf_step[1:])
    return steps


def process_image(image, image_color_space, texture_color_space, width: int, height: int, mip_level: int = 0,
                  type=Type.UNorm, filter=ResizeFilter.CatmullRom, rotate: Optional[RotateAngle] = None,
                  grayscale: bool = False, normal_map: Optional[Tuple[NormalOptions, float]] = None,
                  flip_x: bool = False, flip_y: bool = False, swizzle: Optional[Sequence[Channel]] = None,
                  premultiply: bool = False, orig_image_format=ImageFormat.Invalid, device_id: int = 0,
                  bleed: Optional[dict] = None, sdf: Optional[dict] = None, ao: Optional[dict] = None) -> np.ndarray:
    """loadAndProcessImage (tool/main.cpp:147-277) after the load: colour-space change, resize to the target size
    (max(1, size >> mip_level); the full size first when a normal map is made), rotation, grayscale, normal map
    (normal_map = (NormalOptions, height); KeepSign added for signed types; resized to the mip size afterwards),
    X then Y flip, swizzle, premultiplication and Texture.adjust_image_value_range.  The intermediates stay on the
    device.  Returns the RGBA32F array for Texture.set_image.  image: an (h, w, 4) array or an Image (its pixels).
    bleed = dict(threshold=, wrap=, max_distance=) runs alpha bleeding (Image.bleed_alpha) after the ops pass in front
    of the resize to the texture's size and before that resize (plan_process_image); not with premultiply.
    sdf = dict(spread=, threshold=, wrap=, channels=) writes a signed distance field (Image.distance_field) over the
    named channels of the resized image: the classes come from the alpha in front of that resize, after the ops pass
    there and the bleed, at a scale of source size / target size, which must be 1, 2, 4, 8 or 16 on both axes; not with
    premultiply.
    ao = dict(radius=, height=, directions=, channel=, channels=, strength=, bias=, uniform=, falloff=, wrap=) writes
    the ambient occlusion of the height channel (Image.ambient_occlusion) into the named channels, in front of the
    resize to the texture's size, after the bleed; not with normal_map."""
    if isinstance(image, Image):
        image = image.pixels
    pixels = _pixels(image)
    if ImageFormat(orig_image_format) == ImageFormat.Invalid:
        orig_image_format = ImageFormat.RGBA8 if pixels.dtype == np.uint8 else ImageFormat.RGBAF
    steps = plan_process_image(width, height, pixels.shape[1], pixels.shape[0], image_color_space,
                               texture_color_space, mip_level, type, rotate, grayscale, normal_map, flip_x, flip_y,
                               swizzle, premultiply, bleed, sdf, ao)
    d = _Device(device_id)
    buf = d.upload(pixels)
    for s in steps:
        if s[0] == "ops":
            buf = d.ops(buf, s[1])
        elif s[0] == "bleed":
            buf = d.bleed(buf, s[1], s[2], s[3])
        elif s[0] == "ao":
            buf = d.ao(buf, buf, s[1], **s[2])
        elif s[0] == "sdf_class":
            classes = buf
        elif s[0] == "sdf":
            buf = d.sdf(classes, buf, s[1], s[3], s[4], s[5])
        else:
            buf = d.resize(buf, s[1], s[2], s[3], filter)
    out = d.download(buf)
    if normal_map is not None:
        orig_image_format = ImageFormat.RGBF          # the image no longer matches the original input
    return Texture.adjust_image_value_range(out, type, orig_image_format)
