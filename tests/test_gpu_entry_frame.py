"""What every entry point of the C ABI leaves behind after one successful call at its smallest shape: return code 0, the
kernel name in cfhip_last_kernel_name, the event pairs cfhip_profile_end counts and a time in cfhip_last_kernel_ms --
one call per family that runs through the shared entry frame (guarded), event reset (begin_call) and timed launch
(timed) of csrc/cfhip_api.hip.  Mip generation (2-D, array, 3-D) and resize time nothing and name no kernel: they leave
both as the call before left them.  The literals are the library's behaviour from before the families shared that code.
One more rule came with the shared frame: a successful mip generation or resize clears the context's error text."""
import ctypes

import numpy as np
import pytest

from cuttlefish_amd import ColorSpace, Format, PixelType, Quality, Type, api

pytestmark = pytest.mark.gpu

BC1, RGBA, PVR = Format.BC1_RGB, Format.R8G8B8A8, Format.PVRTC1_RGBA_4BPP
U8 = PixelType.RGBA8


def _pattern(w, h, layers=1):
    """distinct, reproducible texels with every alpha from transparent to opaque"""
    n = layers*h*w*4
    return (np.arange(n, dtype=np.uint32)*37 % 251).astype(np.uint8).reshape(layers, h, w, 4)


class Bufs:
    """the inputs of every call, on the host and on the device, made once"""

    def __init__(self, ctx):
        import torch
        self.torch = torch
        self.img8 = _pattern(8, 8)[0]
        self.img4 = np.ascontiguousarray(self.img8[:4, :4])
        self.two8, self.two4 = _pattern(8, 8, 2), _pattern(4, 4, 2)
        low = api.make_params(BC1, Type.UNorm, Quality.Low)
        self.bc1_8 = ctx.encode([self.img8], low)[0]           # 4 blocks
        self.bc1_4 = ctx.encode([self.img4], low)[0]           # 1 block
        self.pvr_8 = ctx.encode_pvrtc([self.img8], api.make_params(PVR, Type.UNorm, Quality.Low))[0]
        self.d_img8, self.d_img4, self.d_bc1_4 = self.dev(self.img8), self.dev(self.img4), self.dev(self.bc1_4)
        self.d_two8, self.d_two4 = self.dev(self.two8), self.dev(self.two4)

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def zeros(self, *shape, dtype="float32"):
        return self.torch.zeros(shape, dtype=getattr(self.torch, dtype), device="cuda")


@pytest.fixture(scope="module")
def bufs(gpu_ctx):
    b = Bufs(gpu_ctx)
    b.torch.cuda.synchronize()
    return b


def _encode_device(ctx, b):
    out = b.zeros(32, dtype="uint8")
    ctx.encode_device([dict(pixels=b.d_img8.data_ptr(), pixel_type=U8, width=8, height=8, row_pitch_bytes=32,
                            out=out.data_ptr(), out_capacity=32)], api.make_params(BC1, Type.UNorm, Quality.Low))


def _mip_post(ctx, b):
    lv = [b.zeros(2, 2, 4), b.zeros(2, 2, 4)]
    res = b.zeros(2*16, dtype="uint8")
    ctx.mip_post_device([b.d_two4[0].data_ptr(), b.d_two4[1].data_ptr()], U8, 4, 4, 16,
                        [[lv[0].data_ptr()], [lv[1].data_ptr()]], alpha_coverage=0.5, results=res.data_ptr())


def _alpha_bleed(ctx, b):
    work = b.d_two8.clone()
    ctx.alpha_bleed_device([work[0].data_ptr(), work[1].data_ptr()], U8, 8, 8, 32, threshold=0.5)


def _alpha_sdf(scale):
    def call(ctx, b):
        out = b.zeros(2, 8//scale, 8//scale, 4, dtype="uint8")
        ctx.alpha_sdf_device([b.d_two8[0].data_ptr(), b.d_two8[1].data_ptr()], U8, 8, 8, 32,
                             [out[0].data_ptr(), out[1].data_ptr()], U8, (8//scale)*4, spread=2, scale=scale)
    return call


def _spec_aa(w, h, layers, levels_count):
    def call(ctx, b):
        nrm = b.dev(_pattern(w, h, layers))
        lv = [[b.zeros(max(1, h >> k), max(1, w >> k), 4) for k in range(1, levels_count)] for _ in range(layers)]
        ctx.specular_aa_device([nrm[l].data_ptr() for l in range(layers)], U8, w, h, w*4,
                               [[t.data_ptr() for t in chain] for chain in lv], channel=1)
    return call


def _equirect_to_cube(ctx, b):
    faces = b.zeros(6, 2, 2, 4)
    ctx.equirect_to_cube_device(b.d_img8.data_ptr(), U8, 8, 4, 32, [faces[f].data_ptr() for f in range(6)], 2)


def _cube_prefilter(ctx, b):
    src = [b.zeros(6, n, n, 4) for n in (4, 2, 1)]
    dst = [b.zeros(6, n, n, 4) for n in (4, 2)]
    ctx.cube_prefilter_device([[s[f].data_ptr() for s in src] for f in range(6)], 4,
                              [[d[f].data_ptr() for d in dst] for f in range(6)],
                              [None, api.ggx_sample_table(0.5, 64, 4, 3)])


def _cube_sh9(ctx, b):
    faces, res = b.zeros(6, 2, 2, 4), b.zeros(37, dtype="float64")
    ctx.cube_sh9_device([faces[f].data_ptr() for f in range(6)], 2, res.data_ptr())


def _image_ops(ctx, b):
    dst = b.zeros(8, 8, 4)
    ctx.image_ops_device(b.d_img8.data_ptr(), U8, 8, 8, 32, api.make_image_ops(ops=api.ImageOp.FlipX), dst.data_ptr(), 128)


def _decode_device(ctx, b):
    out = b.zeros(4, 4, 4, dtype="uint8")
    ctx.decode_device(b.d_bc1_4.data_ptr(), BC1, Type.UNorm, 4, 4, out.data_ptr(), 16)


# family -> (the call, cfhip_last_kernel_name after it, the event pairs of one call)
TIMED = {
    "encode": (lambda c, b: c.encode([b.img8], api.make_params(BC1, Type.UNorm, Quality.Low)), "cfhip_bc15_encode_kernel", 1),
    "encode_device": (_encode_device, "cfhip_bc15_encode_kernel", 1),
    "alpha_coverage": (lambda c, b: c.alpha_coverage(b.img8, 0.5), "cfhip_mip_post_gather_kernel", 1),
    # gather, decide, six search passes of count + decide, apply
    "mip_post": (_mip_post, "cfhip_mip_post_count_kernel", 15),
    # seed, the steps 4, 2, 1 of an 8 x 8 flood, fill
    "alpha_bleed": (_alpha_bleed, "cfhip_alpha_bleed_step_kernel", 5),
    # classes, row distances, columns; above scale 1 the tiles too
    "alpha_sdf": (_alpha_sdf(1), "cfhip_alpha_sdf_column_kernel", 3),
    "alpha_sdf_scale2": (_alpha_sdf(2), "cfhip_alpha_sdf_column_kernel", 4),
    # one launch per five levels: 64 x 2 has six, the second launch reads the first one's moments
    "spec_aa": (_spec_aa(4, 4, 2, 3), "cfhip_spec_aa_texel_kernel", 1),
    "spec_aa_two_stages": (_spec_aa(64, 2, 1, 7), "cfhip_spec_aa_texel_kernel", 2),
    "equirect_to_cube": (_equirect_to_cube, "cfhip_equirect_to_cube_kernel", 1),
    # one span per destination level: a copy, then 64 samples
    "cube_prefilter": (_cube_prefilter, "cfhip_cube_prefilter_kernel", 2),
    "cube_sh9": (_cube_sh9, "cfhip_cube_sh9_rows_kernel", 2),
    "image_ops": (_image_ops, "cfhip_image_ops_kernel", 1),
    "decode": (lambda c, b: c.decode(b.bc1_4, BC1, Type.UNorm, 4, 4), "cfhip_decode_block_kernel", 1),
    "decode_device": (_decode_device, "cfhip_decode_block_kernel", 1),
    "decode_sse": (lambda c, b: c.decode_sse(b.bc1_4, b.img4, BC1), "cfhip_decode_sse_block_kernel", 1),
    "decode_batch": (lambda c, b: c.decode_batch([b.bc1_4], BC1, Type.UNorm, [(4, 4)]), "cfhip_decode_batch_kernel", 1),
    "compare": (lambda c, b: c.compare(b.bc1_4, b.img4, BC1), "cfhip_compare_block_kernel", 1),
    # Pass A and the reduction; no SSIM pass
    "compare_batch": (lambda c, b: c.compare_batch([b.bc1_4], [b.img4], BC1), "cfhip_compare_batch_block_kernel", 2),
    "rdo": (lambda c, b: c.rdo([b.bc1_8], [b.img8], BC1, Type.UNorm, 1.0), "cfhip_rdo_kernel", 1),
    # the estimate of the plain payloads (five pairs), then one trial, its pass and its estimate: four blocks do not
    # reach the target, so the search ends there
    "rdo_target": (lambda c, b: c.rdo_target([b.bc1_8], [b.img8], BC1, Type.UNorm, 0.9, 32.0), "cfhip_rdo_kernel", 11),
    "deflate_code_lengths": (lambda c, b: c.deflate_code_lengths(np.arange(1, 20, dtype=np.uint32), 7),
                             "cfhip_deflate_emit_kernel", 1),
    # load, init, modulation, one sweep of four phases at Quality.Low, pack
    "pvrtc_encode": (lambda c, b: c.encode_pvrtc([b.img8], api.make_params(PVR, Type.UNorm, Quality.Low)),
                     "cfhip_pvrtc_refine_kernel", 8),
    "pvrtc_decode": (lambda c, b: c.decode_pvrtc(b.pvr_8, PVR, 8, 8), "cfhip_pvrtc_decode_kernel", 1),
    "pvrtc_decode_sse": (lambda c, b: c.decode_pvrtc_sse(b.pvr_8, b.img8, PVR), "cfhip_pvrtc_decode_sse_kernel", 1),
    "std_unpack": (lambda c, b: c.unpack(b.img4, RGBA, Type.UNorm, 4, 4), "cfhip_std_unpack_kernel", 1),
    "std_compare": (lambda c, b: c.compare_std(b.img4, b.img4, RGBA), "cfhip_std_compare_kernel", 1),
}


def _generate_mips(ctx, b):
    lvl = b.zeros(2, 2, 4)
    ctx.generate_mips_device(b.d_img4.data_ptr(), U8, 4, 4, 16, [lvl.data_ptr()])


def _generate_mips_array(ctx, b):
    lv = [b.zeros(2, 2, 4), b.zeros(2, 2, 4)]
    ctx.generate_mips_array_device([b.d_two4[0].data_ptr(), b.d_two4[1].data_ptr()], U8, 4, 4, 16,
                                   [[lv[0].data_ptr()], [lv[1].data_ptr()]])


def _generate_mips3d(ctx, b):
    lvl = b.zeros(1, 2, 2, 4)
    ctx.generate_mips3d_device(b.d_two4.data_ptr(), U8, 4, 4, 2, 16, 64, [lvl.data_ptr()])


def _resize(ctx, b):
    dst = b.zeros(2, 2, 4)
    ctx.resize_device(b.d_img4.data_ptr(), U8, 4, 4, 16, dst.data_ptr(), 2, 2, ColorSpace.Linear)


UNTIMED = {"generate_mips": _generate_mips, "generate_mips_array": _generate_mips_array,
           "generate_mips3d": _generate_mips3d, "resize": _resize}


@pytest.mark.parametrize("family", sorted(TIMED))
def test_a_timed_family_names_its_kernel_and_counts_its_launches(gpu_ctx, bufs, family):
    call, kernel, launches = TIMED[family]
    gpu_ctx.profile_begin()
    try:
        call(gpu_ctx, bufs)                                    # raises unless the return code is 0
        name, ms = gpu_ctx.last_kernel_name(), gpu_ctx.last_kernel_ms()
    finally:
        total, n = gpu_ctx.profile_end()
    print(family, name, n, ms, total)
    assert name == kernel
    assert n == launches
    assert ms >= 0.0 and total >= 0.0
    # outside a profile the call's own pairs are all there is
    call(gpu_ctx, bufs)
    assert gpu_ctx.last_kernel_name() == kernel and gpu_ctx.last_kernel_ms() >= 0.0


@pytest.mark.parametrize("family", sorted(UNTIMED))
def test_mip_generation_and_resize_leave_name_and_time_alone(gpu_ctx, bufs, family):
    _image_ops(gpu_ctx, bufs)
    name, ms = gpu_ctx.last_kernel_name(), gpu_ctx.last_kernel_ms()
    assert name == "cfhip_image_ops_kernel" and ms >= 0.0
    UNTIMED[family](gpu_ctx, bufs)
    assert gpu_ctx.last_kernel_name() == name
    assert gpu_ctx.last_kernel_ms() == ms                      # the same pair of events, read again
    gpu_ctx.profile_begin()
    try:
        _image_ops(gpu_ctx, bufs)
        UNTIMED[family](gpu_ctx, bufs)
    finally:
        total, n = gpu_ctx.profile_end()
    print(family, n, total)
    assert n == 1 and total >= 0.0                             # the image ops' pair alone
    assert gpu_ctx.last_kernel_name() == name


@pytest.mark.parametrize("family", sorted(UNTIMED))
def test_a_successful_mip_generation_or_resize_clears_the_error_text(gpu_ctx, bufs, family):
    """the one rule here that the library did not follow before these four shared the entry frame"""
    last_error = lambda: gpu_ctx._lib.cfhip_last_error(gpu_ctx._h)
    with pytest.raises(api.CfhipError, match="decode: empty surface 0x4"):
        gpu_ctx.decode(bufs.bc1_4, BC1, Type.UNorm, 0, 4)
    assert last_error() == b"decode: empty surface 0x4"
    UNTIMED[family](gpu_ctx, bufs)
    assert last_error() == b""
