"""GPU image ops (csrc/image_ops.hip, cfhip_image_ops_device) against tests/image_ref.py, the reference's ImageTest
cases through cuttlefish_amd.Image, one fused call against the same ops one call each, process_image against a numpy
run of the tool's order, the all-device chain into the mip generator and the encoder, and argument errors."""
import ctypes

import numpy as np
import pytest

import image_ref as R
import test_image_ref as T

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 19), (19, 1), (37, 23), (256, 192)]
PIXELS = ["u8", "f32", "f16"]


def _image(w, h, kind, seed=0):
    rng = np.random.default_rng(seed + 7 * w + h)
    if kind == "u8":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    v = rng.random((h, w, 4)) * 1.05 - 0.02           # a little outside [0, 1] too
    return v.astype(np.float16 if kind == "f16" else np.float32)


def _run(ctx, img, ops):
    import torch
    from cuttlefish_amd import api
    host = np.ascontiguousarray(img)
    src = torch.from_numpy(host).cuda()
    h, w = host.shape[:2]
    quarter = (ops.ops & api.ImageOp.Rotate) and ops.rotate not in (1, 4)
    rw, rh = (h, w) if quarter else (w, h)
    dst = torch.empty((rh, rw, 4), dtype=torch.float32, device="cuda")
    ctx.image_ops_device(src.data_ptr(), api.pixel_type_of(host), w, h, host.strides[0], ops, dst.data_ptr(), rw * 16)
    return dst.cpu().numpy()


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


OPS_ALONE = ["flip_x", "flip_y", "rot_cw90", "rot_180", "rot_ccw90", "swizzle", "swizzle_none", "grayscale",
             "premultiply", "to_other_space", "normal", "normal_keep", "normal_wrap_x", "normal_wrap_y",
             "normal_wrap_xy_keep"]


def _desc(name, cs):
    from cuttlefish_amd import api
    Op = api.ImageOp
    if name.startswith("rot"):
        angle = {"rot_cw90": R.CW90, "rot_180": R.CW180, "rot_ccw90": R.CCW90}[name]
        return dict(ops=Op.Rotate, rotate=angle), dict(rot=angle)
    if name.startswith("normal"):
        opt = {"normal": 0, "normal_keep": R.KEEP_SIGN, "normal_wrap_x": R.WRAP_X, "normal_wrap_y": R.WRAP_Y,
               "normal_wrap_xy_keep": R.WRAP_X | R.WRAP_Y | R.KEEP_SIGN}[name]
        return (dict(ops=Op.NormalMap, normal_options=opt, normal_height=2.5),
                dict(normal_options=opt, normal_height=2.5))
    if name.startswith("swizzle"):
        swz = (R.ALPHA, R.BLUE, R.RED, R.GREEN) if name == "swizzle" else (R.GREEN, R.NONE, R.RED, R.NONE)
        return dict(ops=Op.Swizzle, swizzle=swz), dict(swz=swz)
    if name == "to_other_space":
        return dict(ops=Op.ColorSpace, dst_color_space=1 - cs), dict(dst_cs=1 - cs)
    bit = {"flip_x": Op.FlipX, "flip_y": Op.FlipY, "grayscale": Op.Grayscale, "premultiply": Op.PreMultiply}[name]
    return dict(ops=bit), {}


@pytest.mark.parametrize("cs", [0, 1], ids=["linear", "srgb"])
@pytest.mark.parametrize("kind", PIXELS)
@pytest.mark.parametrize("name", OPS_ALONE)
def test_each_op_alone_matches_image_ref(gpu_ctx, name, kind, cs):
    from cuttlefish_amd import api
    dev, ref = _desc(name, cs)
    ops = api.make_image_ops(src_color_space=cs, **dev)
    for w, h in SIZES:
        img = _image(w, h, kind)
        got = _run(gpu_ctx, img, ops)
        want = R.apply_ops(img, int(dev["ops"]), src_cs=cs, **ref)
        assert got.shape == want.shape, (w, h)
        uses_pow = cs == R.SRGB and name in ("grayscale", "premultiply") or name == "to_other_space"
        if name.startswith("normal"):
            d = _ulps(got, want)
            print("%s %s %dx%d: %d of %d values differ, max %d ulp" % (name, kind, w, h, int((d > 0).sum()), d.size,
                                                                      int(d.max())))
            assert d.max() <= 1, (w, h)
        elif uses_pow:
            assert _ulps(got, want).max() <= 2, (w, h)
        else:
            assert np.array_equal(got, want), (w, h)


@pytest.mark.parametrize("case", T.CASES, ids=[c.__name__[5:] for c in T.CASES])
def test_imagetest_cases_through_image(gpu_ctx, case):
    from cuttlefish_amd import Image
    case(Image)


def test_fused_equals_chained(gpu_ctx):
    """every op on, one call, against the same ops one call each (the float stores between ops pinned); 4096 x 2048,
    every rotate angle and wrap flag, RGBA8 and RGBA32F sources; compared on the device"""
    import torch
    from cuttlefish_amd import api
    Op = api.ImageOp
    order = [Op.ColorSpace, Op.Rotate, Op.Grayscale, Op.NormalMap, Op.FlipX, Op.FlipY, Op.Swizzle, Op.PreMultiply]
    w, h = 4096, 2048
    for kind in ("u8", "f32"):
        host = _image(w, h, kind, seed=1)
        src = torch.from_numpy(host).cuda()
        pt = api.pixel_type_of(host)
        for normal in (False, True):
            for angle in range(6):
                for wrap in ((0, R.WRAP_X, R.WRAP_Y, R.WRAP_X | R.WRAP_Y) if normal else (0,)):
                    common = dict(rotate=angle, normal_options=wrap, normal_height=1.7,
                                  swizzle=(R.ALPHA, R.BLUE, R.NONE, R.RED))
                    mask = [o for o in order if normal or o != Op.NormalMap]
                    quarter = angle not in (1, 4)
                    rw, rh = (h, w) if quarter else (w, h)
                    fused = torch.empty((rh, rw, 4), dtype=torch.float32, device="cuda")
                    # odd angles stay sRGB: grayscale then reads the 8-bit table in the fused call, pow() chained
                    tcs = angle % 2
                    ops = api.make_image_ops(sum(int(o) for o in mask), src_color_space=1, dst_color_space=tcs,
                                             **common)
                    gpu_ctx.image_ops_device(src.data_ptr(), pt, w, h, host.strides[0], ops, fused.data_ptr(), rw * 16)
                    cur, cur_pt, cw, ch, pitch = src, pt, w, h, host.strides[0]
                    cs, rgbf = 1, False
                    for o in mask:
                        ow, oh = (ch, cw) if o == Op.Rotate and quarter else (cw, ch)
                        out = torch.empty((oh, ow, 4), dtype=torch.float32, device="cuda")
                        one = api.make_image_ops(o, src_color_space=cs, dst_color_space=tcs, rgbf=rgbf, **common)
                        gpu_ctx.image_ops_device(cur.data_ptr(), cur_pt, cw, ch, pitch, one, out.data_ptr(), ow * 16)
                        cs = tcs if o == Op.ColorSpace else cs
                        rgbf = rgbf or o == Op.NormalMap
                        cur, cur_pt, cw, ch, pitch = out, api.PixelType.RGBA32F, ow, oh, ow * 16
                    torch.cuda.synchronize()
                    assert torch.equal(fused.view(torch.int32), cur.view(torch.int32)), (kind, normal, angle, wrap)


def _tool_order(ctx, img, ics, tcs, width, height, mip, typ, rotate, gray, normal, flip_x, flip_y, swz, premul):
    """loadAndProcessImage restated with image_ref, one op at a time, the resizes through Image.resize"""
    from cuttlefish_amd import Image, Texture
    from cuttlefish_amd.texture import ImageFormat
    orig = ImageFormat.RGBA8 if img.dtype == np.uint8 else ImageFormat.RGBAF
    a = R.to_rgbaf(img)
    cs = ics
    if tcs != ics:
        a = R.change_color_space(a, ics, tcs)
        cs = tcs
    tw, th = max(width >> mip, 1), max(height >> mip, 1)
    nw, nh = (width, height) if normal else (tw, th)
    if (nw, nh) != (a.shape[1], a.shape[0]):
        a = Image(a, cs).resize(nw, nh).pixels
    if rotate is not None:
        a = R.rotate(a, rotate)
    if gray:
        a = R.grayscale(a, cs)
    rgbf = False
    if normal:
        opt = normal[0] | (R.KEEP_SIGN if typ in (1, 3, 5) else 0)
        a = R.normal_map(a, opt, normal[1])
        if (nw, nh) != (tw, th):
            a = Image(a, cs).resize(tw, th).pixels
            a[..., 3] = 1.0
        rgbf = True
        orig = ImageFormat.RGBF
    if flip_x:
        a = R.flip_horizontal(a)
    if flip_y:
        a = R.flip_vertical(a)
    if swz:
        a = R.swizzle(a, swz, rgbf)
    if premul:
        a = R.pre_multiply_alpha(a, cs, rgbf)
    return Texture.adjust_image_value_range(a, typ, orig)


PROCESS = [
    dict(size=(50, 40), width=32, height=32, mip=0, normal=None),
    dict(size=(50, 40), width=32, height=32, mip=2, normal=None),
    dict(size=(32, 32), width=32, height=32, mip=0, normal=(R.WRAP_X, 3.0)),
    dict(size=(50, 40), width=32, height=32, mip=0, normal=(0, 3.0)),
    dict(size=(50, 40), width=32, height=32, mip=2, normal=(R.WRAP_Y, 3.0)),
    dict(size=(32, 16), width=32, height=16, mip=2, normal=(0, 2.0), typ=1),          # SNorm: KeepSign
    dict(size=(24, 24), width=24, height=24, mip=0, normal=(0, 2.0), swz=(R.ALPHA, R.RED, R.GREEN, R.BLUE),
         premul=True),
    dict(size=(24, 24), width=24, height=24, mip=0, normal=None, typ=1, premul=True, rotate=R.CW90),
]


@pytest.mark.parametrize("p", PROCESS, ids=[str(i) for i in range(len(PROCESS))])
def test_process_image_follows_the_tool_order(gpu_ctx, p):
    from cuttlefish_amd import process_image
    img = _image(p["size"][0], p["size"][1], "u8", seed=4)
    typ = p.get("typ", 0)
    kw = dict(rotate=p.get("rotate"), grayscale=True, flip_x=True, flip_y=True, swizzle=p.get("swz"),
              premultiply=p.get("premul", False))
    got = process_image(img, 1, 0, p["width"], p["height"], mip_level=p["mip"], type=typ, normal_map=p["normal"],
                        **kw)
    want = _tool_order(gpu_ctx, img, 1, 0, p["width"], p["height"], p["mip"], typ, kw["rotate"], True, p["normal"],
                       True, True, kw["swizzle"], kw["premultiply"])
    assert got.shape == want.shape
    # pow() differs in the last bit from libm's, and a resize or a normal map after it carries that on
    assert np.abs(got.astype(np.float64) - want).max() <= 1e-5
    if p["normal"] is not None:
        assert np.all(got[..., 3] == 1.0)                 # RGBF: alpha 1 after swizzle, premultiply, resize
        if typ == 0:
            assert got.min() >= 0.0                       # not remapped to [-1, 1]: orig format is RGBF now


@pytest.mark.parametrize("case", ["bc5_normal", "bc7_srgb_premultiplied"])
def test_device_chain_matches_host_route(gpu_ctx, case):
    """image_ops_device -> generate_mips_device -> encode_device on device buffers, against process_image ->
    Texture.generate_mipmaps -> convert"""
    import torch
    from cuttlefish_amd import Format, Texture, Type, api, make_params, payload_size, process_image
    img = _image(64, 48, "u8", seed=9)
    if case == "bc5_normal":
        fmt, typ, cs, kw = Format.BC5, Type.SNorm, 0, dict(normal_map=(R.WRAP_X | R.KEEP_SIGN, 4.0))
        ops = api.make_image_ops(api.ImageOp.NormalMap, normal_options=R.WRAP_X | R.KEEP_SIGN, normal_height=4.0)
    else:
        fmt, typ, cs, kw = Format.BC7, Type.UNorm, 1, dict(premultiply=True, flip_y=True)
        ops = api.make_image_ops(api.ImageOp.PreMultiply | api.ImageOp.FlipY, src_color_space=1)
    levels = 4
    host = process_image(img, cs, cs, 64, 48, type=typ, **kw)
    tex = Texture(64, 48, mip_levels=levels, color_space=cs)
    assert tex.set_image(host)
    assert tex.generate_mipmaps(api.ResizeFilter.Box, mip_levels=levels)
    assert tex.convert(fmt, typ)
    want = [tex.data(m) for m in range(levels)]
    src = torch.from_numpy(img).cuda()
    lv = [torch.empty((max(48 >> k, 1), max(64 >> k, 1), 4), dtype=torch.float32, device="cuda") for k in range(levels)]
    gpu_ctx.image_ops_device(src.data_ptr(), api.PixelType.RGBA8, 64, 48, 256, ops, lv[0].data_ptr(), 64 * 16)
    gpu_ctx.generate_mips_device(lv[0].data_ptr(), api.PixelType.RGBA32F, 64, 48, 64 * 16,
                                 [t.data_ptr() for t in lv[1:]], color_space=cs, filter=0)
    params = make_params(fmt, typ, color_space=cs)
    outs = [torch.zeros(payload_size(fmt, typ, t.shape[1], t.shape[0]), dtype=torch.uint8, device="cuda") for t in lv]
    gpu_ctx.encode_device([dict(pixels=t.data_ptr(), pixel_type=api.PixelType.RGBA32F, width=t.shape[1],
                                height=t.shape[0], row_pitch_bytes=t.shape[1] * 16, out=o.data_ptr(),
                                out_capacity=o.numel()) for t, o in zip(lv, outs)], params)
    torch.cuda.synchronize()
    for k in range(levels):
        assert np.array_equal(outs[k].cpu().numpy(), np.asarray(want[k]).reshape(-1)), k


def test_argument_errors_launch_nothing(gpu_ctx):
    import torch
    from cuttlefish_amd import CfhipError, Format, Type, api, make_params, synth
    L = api.load_library()
    src = torch.zeros((8, 16, 4), dtype=torch.float32, device="cuda")
    dst = torch.full((8, 16, 4), 7.0, dtype=torch.float32, device="cuda")
    good = api.make_image_ops(api.ImageOp.FlipX)

    def call(s=src.data_ptr(), pt=1, w=16, h=8, pitch=256, ops=good, d=dst.data_ptr(), dpitch=256):
        rc = L.cfhip_image_ops_device(gpu_ctx._h, ctypes.c_void_p(s) if s else None, pt, w, h, pitch,
                                      ctypes.byref(ops) if ops is not None else None,
                                      ctypes.c_void_p(d) if d else None, dpitch, None)
        return rc, L.cfhip_last_error(gpu_ctx._h).decode()

    def bad(**f):
        o = api.make_image_ops(api.ImageOp.FlipX)
        for k, v in f.items():
            if k == "swizzle0":
                o.swizzle[0] = v
            else:
                setattr(o, k, v)
        return o

    cases = [dict(s=0), dict(d=0), dict(ops=None), dict(w=0), dict(h=0), dict(pt=3), dict(pitch=255),
             dict(dpitch=128), dict(ops=bad(ops=1 << 8)), dict(ops=bad(src_color_space=2)),
             dict(ops=bad(dst_color_space=-1)), dict(ops=bad(rotate=6)), dict(ops=bad(normal_options=8)),
             dict(ops=bad(swizzle0=5)), dict(ops=bad(rgbf=2)), dict(d=src.data_ptr() + 64),
             dict(d=src.data_ptr())]
    for c in cases:
        rc, text = call(**c)
        assert rc == api.E_INVALID and text, c
    torch.cuda.synchronize()
    assert torch.all(dst == 7.0)                        # nothing was launched
    img = synth.photo(16, 16, seed=2)
    got = gpu_ctx.encode([img], make_params(Format.BC1_RGB, Type.UNorm))[0]
    import oracle_lib as O
    assert np.array_equal(got, O.encode(img, int(Format.BC1_RGB), quality=2, threads=1))
    with pytest.raises(CfhipError):
        gpu_ctx.image_ops_device(src.data_ptr(), 1, 16, 8, 256, bad(rotate=9), dst.data_ptr(), 256)


def test_stream_rule_on_a_callers_stream(gpu_ctx):
    import torch
    from cuttlefish_amd import api
    img = _image(300, 200, "f32", seed=3)
    src = torch.from_numpy(img).cuda()
    dst = torch.empty((300, 200, 4), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    ops = api.make_image_ops(api.ImageOp.Rotate | api.ImageOp.FlipY, rotate=R.CCW90)
    with torch.cuda.stream(s):
        gpu_ctx.image_ops_device(src.data_ptr(), 1, 300, 200, 300 * 16, ops, dst.data_ptr(), 200 * 16,
                                 stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(dst.cpu().numpy(), R.flip_vertical(R.rotate(img, R.CCW90)))
    assert gpu_ctx.last_kernel_ms() >= 0.0
