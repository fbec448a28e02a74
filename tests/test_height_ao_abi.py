"""cfhip_height_ao_array_device without a GPU: the exports, the two structs against the header's text, the flags in
header, api and twin, the direction table against the twin's, every argument error -- each returns before any device
call, a NULL context last -- and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import height_ao_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cfhip_height_ao_array_device"
TABLE = "cfhip_height_ao_directions"
KERNELS = ("cfhip_height_ao_plane_kernel", "cfhip_height_ao_scan_kernel")


def test_exports_and_structs(hip_lib):
    from cuttlefish_amd import api, build
    from test_abi import _declared_symbols
    from test_lz4_abi import _struct_fields
    for name in (NAME, TABLE):
        assert name in api.EXPORTS and name in _declared_symbols() and hasattr(hip_lib, name)
    assert hip_lib.cfhip_abi_version() == 1
    P, R = api.HeightAoParams, api.HeightAoResult
    fields = [("uint32_t", "struct_size"), ("uint32_t", "flags"), ("uint32_t", "channel"), ("uint32_t", "directions"),
              ("uint32_t", "radius"), ("uint32_t", "channel_mask"), ("float", "height"), ("float", "strength"),
              ("float", "bias"), ("uint32_t", "reserved")]
    assert ctypes.sizeof(P) == 40 and ctypes.sizeof(R) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [(n, 4*i) for i, (_, n) in enumerate(fields)]
    assert _struct_fields("cfhip_height_ao_params") == fields
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [("occluded", 0), ("darkest", 4), ("reserved", 8)]
    assert _struct_fields("cfhip_height_ao_result") == [("uint32_t", "occluded"), ("uint32_t", "darkest"),
                                                        ("uint32_t", "reserved[2]")]
    assert api.HEIGHT_AO_RESULT_DTYPE.itemsize == 16 and api.HEIGHT_AO_RESULT_DTYPE.names == height_ao_ref.FIELDS
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    flags = re.search(r"enum \{ CFHIP_HAO_WRAP_X = (\d+), CFHIP_HAO_WRAP_Y = (\d+), CFHIP_HAO_UNIFORM = (\d+), "
                      r"CFHIP_HAO_FALLOFF = (\d+) \};", header)
    assert tuple(int(v) for v in flags.groups()) \
        == (api.HAO_WRAP_X, api.HAO_WRAP_Y, api.HAO_UNIFORM, api.HAO_FALLOFF) \
        == (height_ao_ref.WRAP_X, height_ao_ref.WRAP_Y, height_ao_ref.UNIFORM, height_ao_ref.FALLOFF) == (1, 2, 4, 8)
    assert NAME in re.search(r"/\* Kernel-only time of the most recent.*?\*/", header, re.S).group(0)
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "height_ao.h")).read()
    assert int(re.search(r"CFHAO_MAX_SIDE = (\d+);", shared).group(1)) == height_ao_ref.MAX_SIDE == 32768
    assert int(re.search(r"CFHAO_MAX_RADIUS = (\d+);", shared).group(1)) == height_ao_ref.MAX_RADIUS \
        == api.HAO_MAX_RADIUS == 64
    assert "2 plain launches" in header[header.index("Ambient occlusion from height maps"):header.index("cfhip_height_ao_params;")]
    for k in KERNELS:
        assert k in build.BLOCK_KERNELS


def test_direction_table_equals_the_twins(hip_lib):
    from cuttlefish_amd import api
    for D in (8, 16, 32):
        vx, vy, w = api.height_ao_directions(D)
        tx, ty, tw = height_ao_ref.directions(D)
        assert vx.dtype == vy.dtype == np.int32 and w.dtype == np.float64
        assert (vx == tx).all() and (vy == ty).all()
        assert np.abs(w - tw).max() <= 2.0**-50
        assert abs(float(np.sum(w)) - 1.0) <= 2.0**-50
        assert height_ao_ref.in_order_sum(w) == 1.0 and (w == tw).all()       # a flat surface is exactly 1
        angle = [0.5*np.arctan2(float(tx[d - 1]*ty[(d + 1) % D] - ty[d - 1]*tx[(d + 1) % D]),
                                float(tx[d - 1]*tx[(d + 1) % D] + ty[d - 1]*ty[(d + 1) % D]))/(2.0*np.pi) for d in range(D)]
        assert np.abs(w - np.array(angle)).max() <= 2.0**-50                  # the weights are the atan2 angles
        # any output may be left out
        only = np.zeros(D, np.float64)
        assert hip_lib.cfhip_height_ao_directions(D, None, None, only.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
        assert (only == w).all()
    for bad in (0, 4, 12, 24, 64):
        assert hip_lib.cfhip_height_ao_directions(bad, None, None, None) == api.E_INVALID
    for bad in (0, 4, 33, True, None):
        with pytest.raises(ValueError):
            api.height_ao_directions(bad)


def test_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    # host memory stands in for the surfaces: no call gets as far as touching them
    W, H = 16, 8
    src = [np.zeros((H, W, 4), np.float32) for _ in range(2)]
    dst = [np.zeros((H, W, 4), np.float32) for _ in range(2)]
    res = np.zeros(2*4, np.uint32)
    ok = dict(src=[a.ctypes.data for a in src], dst=[a.ctypes.data for a in dst], layers=2, spt=1, dpt=1, w=W, h=H,
              sp=W*16, dp=W*16, size=40, flags=15, channel=1, D=16, radius=8, mask=1, height=1.0, strength=1.0, bias=0.0,
              reserved=0, res=res.ctypes.data, params=True)

    def call(**kw):
        a = dict(ok, **kw)
        arr = lambda v: (ctypes.c_void_p*len(v))(*v) if v is not None else None      # noqa: E731
        p = api.HeightAoParams(a["size"], a["flags"], a["channel"], a["D"], a["radius"], a["mask"], a["height"],
                               a["strength"], a["bias"], a["reserved"])
        return hip_lib.cfhip_height_ao_array_device(None, arr(a["src"]), a["layers"], a["spt"], a["w"], a["h"], a["sp"],
                                                    arr(a["dst"]), a["dpt"], a["dp"],
                                                    ctypes.byref(p) if a["params"] else None, a["res"], None)
    # everything right but the context: reported, and reported last
    assert call() == api.E_INVALID and err() == b"ctx is NULL"
    assert call(res=None) == api.E_INVALID and err() == b"ctx is NULL"                 # the records are optional
    assert call(dst=ok["src"]) == api.E_INVALID and err() == b"ctx is NULL"            # in place
    assert call(flags=0, channel=3, D=8, radius=1, mask=15, height=-2.5, strength=0.0, bias=3.0) == api.E_INVALID \
        and err() == b"ctx is NULL"
    assert call(D=32, radius=64, strength=2.5, height=0.0) == api.E_INVALID and err() == b"ctx is NULL"
    for spt, stexel in ((0, 4), (2, 8), (1, 16)):
        for dpt, dtexel in ((0, 4), (2, 8), (1, 16)):
            assert call(spt=spt, sp=W*stexel + stexel//4, dpt=dpt, dp=W*dtexel + dtexel//4) == api.E_INVALID \
                and err() == b"ctx is NULL"
    assert call(w=32768, h=32768, layers=1, sp=32768*16, dp=32768*16) == api.E_INVALID and err() == b"ctx is NULL"
    assert call(params=False) == api.E_INVALID and err() == b"height_ao: params is NULL"
    for size in (0, 32, 36, 44, 80):
        assert call(size=size) == api.E_INVALID and err() == b"height_ao: params->struct_size is %d, not 40" % size
    assert call(src=None) == api.E_INVALID and err() == b"height_ao: src is NULL"
    assert call(dst=None) == api.E_INVALID and err() == b"height_ao: dst is NULL"
    for layers in (0, 65536):
        assert call(layers=layers) == api.E_INVALID and err() == b"height_ao: layers is %d (1 to 65535 per call)" % layers
    for w, h in ((0, 8), (16, 0), (32769, 8), (16, 32769), (0xFFFFFFFE, 2)):
        assert call(w=w, h=h, sp=(1 << 40), dp=(1 << 40)) == api.E_INVALID \
            and err() == b"height_ao: width and height are 1 to 32768 each, not %dx%d" % (w, h)
    for pt in (-1, 3, 99):
        assert call(spt=pt) == api.E_INVALID and err() == b"height_ao: src_pixel_type %d" % pt
        assert call(dpt=pt) == api.E_INVALID and err() == b"height_ao: dst_pixel_type %d" % pt
    for flags in (16, 32, 1 | 64, 0x80000000):
        assert call(flags=flags) == api.E_INVALID and err() == b"height_ao: params->flags 0x%x: unknown" % flags
    for channel in (4, 5, 0xFFFFFFFF):
        assert call(channel=channel) == api.E_INVALID and err() == b"height_ao: params->channel %d above 3" % channel
    for D in (0, 4, 12, 24, 33, 64):
        assert call(D=D) == api.E_INVALID and err() == b"height_ao: params->directions %d is not 8, 16 or 32" % D
    for radius in (0, 65, 128, 0xFFFFFFFF):
        assert call(radius=radius) == api.E_INVALID and err() == b"height_ao: params->radius %d outside 1 to 64" % radius
    for mask in (0, 16, 255):
        assert call(mask=mask) == api.E_INVALID and err() == b"height_ao: params->channel_mask 0x%x outside 1 to 15" % mask
    for bad, text in ((float("nan"), b"nan"), (float("inf"), b"inf"), (float("-inf"), b"-inf")):
        assert call(height=bad) == api.E_INVALID and err() == b"height_ao: params->height %s is not finite" % text
        assert call(strength=bad) == api.E_INVALID and err() == b"height_ao: params->strength %s is negative or not finite" % text
        assert call(bias=bad) == api.E_INVALID and err() == b"height_ao: params->bias %s is negative or not finite" % text
    assert call(strength=-0.5) == api.E_INVALID and err() == b"height_ao: params->strength -0.5 is negative or not finite"
    assert call(bias=-0.25) == api.E_INVALID and err() == b"height_ao: params->bias -0.25 is negative or not finite"
    for reserved in (1, 0x80000000):
        assert call(reserved=reserved) == api.E_INVALID and err() == b"height_ao: params->reserved is %d, not 0" % reserved
    assert call(w=32768, h=32768 + 0, layers=1, sp=32768*16, dp=32768*16) == api.E_INVALID and err() == b"ctx is NULL"
    assert call(w=32768, h=32768, spt=0, sp=32768*4, dp=32768*16, layers=1) == api.E_INVALID and err() == b"ctx is NULL"
    assert call(sp=W*16 - 4) == api.E_INVALID and err() == b"height_ao: src_pitch_bytes 252 < 256, a row"
    assert call(dp=W*16 - 4) == api.E_INVALID and err() == b"height_ao: dst_pitch_bytes 252 < 256, a row"
    assert call(sp=W*16 + 2) == api.E_INVALID \
        and err() == b"height_ao: src_pitch_bytes 258 not aligned to a component (4 bytes)"
    assert call(dpt=2, dp=W*8 + 1) == api.E_INVALID \
        and err() == b"height_ao: dst_pitch_bytes 129 not aligned to a component (2 bytes)"
    assert call(src=[src[0].ctypes.data, None]) == api.E_INVALID and err() == b"height_ao: src[1] is NULL"
    assert call(dst=[None, dst[1].ctypes.data]) == api.E_INVALID and err() == b"height_ao: dst[0] is NULL"
    assert call(src=[src[0].ctypes.data, src[1].ctypes.data + 2]) == api.E_INVALID \
        and err() == b"height_ao: src[1] not aligned to a component (4 bytes)"
    assert call(dst=[dst[0].ctypes.data + 1, dst[1].ctypes.data], dpt=2, dp=W*8) == api.E_INVALID \
        and err() == b"height_ao: dst[0] not aligned to a component (2 bytes)"
    assert call(dst=[dst[0].ctypes.data, src[1].ctypes.data], dpt=0, dp=W*4) == api.E_INVALID \
        and err() == b"height_ao: dst[1] equals src[1]: in place needs equal pixel types"
    assert not res.any() and not any(a.any() for a in src + dst)


def test_more_than_2_30_texels_cannot_be_asked_for():
    # sides of at most 32768 bound a surface at 2^30 texels: the check on the product guards the sides' limit
    assert height_ao_ref.MAX_SIDE**2 == 1 << 30


def test_make_height_ao_params_rejects_every_bad_field():
    from cuttlefish_amd import api
    p = api.make_height_ao_params(8)
    assert (p.struct_size, p.flags, p.channel, p.directions, p.radius, p.channel_mask, p.height, p.strength, p.bias,
            p.reserved) == (40, 0, 0, 16, 8, 1, 1.0, 1.0, 0.0, 0)
    p = api.make_height_ao_params(64, -2.0, 32, "A", "gb", 2.5, 0.125, True, True, (True, False))
    assert (p.flags, p.channel, p.directions, p.radius, p.channel_mask, p.height, p.strength, p.bias) == \
        (1 | 4 | 8, 3, 32, 64, 6, -2.0, 2.5, 0.125)
    assert api.make_height_ao_params(1, wrap=True).flags == 3 and api.make_height_ao_params(1, channels=15).channel_mask == 15
    for bad in (dict(radius=0), dict(radius=65), dict(radius=True), dict(radius=2.0), dict(radius=None),
                dict(directions=4), dict(directions=12), dict(directions=True), dict(directions=None),
                dict(channel="x"), dict(channel=4), dict(channel="rg"), dict(channels=""), dict(channels="rr"),
                dict(channels=0), dict(channels=16), dict(channels="q"),
                dict(height_scale=float("nan")), dict(height_scale=float("inf")), dict(height_scale=1e39),
                dict(strength=-1.0), dict(strength=float("nan")), dict(strength=float("inf")),
                dict(bias=-0.1), dict(bias=float("nan")), dict(bias=float("inf")), dict(bias=1e39)):
        with pytest.raises(ValueError):
            api.make_height_ao_params(**dict(dict(radius=8), **bad))


def test_python_surface():
    from cuttlefish_amd import ColorSpace, Dimension, Image, Texture, api, plan_process_image, process_image
    sig = inspect.signature(api.Context.height_ao_device)
    assert list(sig.parameters)[1:] == ["srcs", "pixel_type", "width", "height", "pitch", "dsts", "dst_pixel_type",
                                        "dst_pitch", "radius", "height_scale", "directions", "channel", "channels",
                                        "strength", "bias", "uniform", "falloff", "wrap", "results", "stream"]
    kw = {n: p.default for n, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY}
    assert kw == dict(radius=inspect.Parameter.empty, height_scale=1.0, directions=16, channel="r", channels="r",
                      strength=1.0, bias=0.0, uniform=False, falloff=False, wrap=(False, False), results=0, stream=0)
    sig = inspect.signature(api.Context.height_ao)
    assert list(sig.parameters)[1:3] == ["image", "radius"] and sig.parameters["out_dtype"].default is None
    sig = inspect.signature(Image.ambient_occlusion)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:3]] == [("radius", inspect.Parameter.empty),
                                                                             ("height", 1.0)]
    sig = inspect.signature(Texture.height_ambient_occlusion)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:4]] == \
        [("heights", inspect.Parameter.empty), ("channel", "r"), ("height_channel", "r")]
    assert callable(Texture.ao_results)
    # what is refused is refused before any device work
    img = np.zeros((4, 4, 4), np.float32)
    assert Image(img, rgbf=True).ambient_occlusion(4) is None
    with pytest.raises(ValueError):
        Image(img).ambient_occlusion(0)
    with pytest.raises(ValueError):
        Image(img).ambient_occlusion(4, directions=12)

    def tex(dim=Dimension.Dim2D, w=4, h=4, depth=0, mips=1):
        t = Texture(dim, w, h, depth, mips)
        for m in range(t.mip_level_count()):
            for d in range(max(t.depth(m), 1)):
                assert t.set_image(np.zeros((max(h >> m, 1), max(w >> m, 1), 4), np.float32), m, d)
        return t
    good = tex()
    assert Texture().height_ambient_occlusion(good, radius=2) is False
    assert good.height_ambient_occlusion(Texture(), radius=2) is False
    assert good.height_ambient_occlusion(img, radius=2) is False and good.ao_results() == []
    assert tex(Dimension.Dim3D, depth=4).height_ambient_occlusion(good, radius=2) is False            # 3-D
    assert good.height_ambient_occlusion(tex(w=8, h=8), radius=2) is False                            # a size mismatch
    assert good.height_ambient_occlusion(tex(w=4, h=8), radius=2) is False
    assert good.height_ambient_occlusion(tex(depth=2), radius=2) is False                             # another depth
    assert good.height_ambient_occlusion(Texture(Dimension.Dim2D, 4, 4, 0, 1), radius=2) is False     # no image to read
    with pytest.raises(ValueError):
        good.height_ambient_occlusion(good, channel="q", radius=2)
    with pytest.raises(ValueError):
        good.height_ambient_occlusion(good, radius=65)
    with pytest.raises(TypeError):
        good.height_ambient_occlusion(good)                 # the radius has no default
    # process_image: the step sits where the bleed step sits, after it; its ValueErrors come before any device work
    args = (12, 10, 24, 20, ColorSpace.sRGB, ColorSpace.Linear)
    steps = plan_process_image(*args, ao=dict(radius=5, height=2.0, wrap=True), bleed={})
    assert [s[0] for s in steps] == ["ops", "bleed", "ao", "resize"]
    assert steps[2][1] == 5 and steps[2][2] == dict(height_scale=2.0, wrap=True)
    assert [s[0] for s in plan_process_image(24, 20, 24, 20, ColorSpace.Linear, ColorSpace.Linear, ao=dict(radius=1))] \
        == ["ops", "ao"]
    assert [s[0] for s in plan_process_image(*args, ao=None)] == [s[0] for s in plan_process_image(*args)] \
        == ["ops", "resize"]
    for bad in (dict(), dict(height=1.0), dict(radius=4, spread=2), dict(radius=4, height_scale=1.0), dict(radius=0),
                dict(radius=4, directions=7), dict(radius=4, strength=-1.0), dict(radius=4, channels="")):
        with pytest.raises(ValueError):
            plan_process_image(*args, ao=bad)
        with pytest.raises(ValueError):
            process_image(np.zeros((20, 24, 4), np.float32), ColorSpace.sRGB, ColorSpace.Linear, 12, 10, ao=bad)
    with pytest.raises(ValueError, match="normal"):
        plan_process_image(*args, ao=dict(radius=4), normal_map=(0, 1.0))
