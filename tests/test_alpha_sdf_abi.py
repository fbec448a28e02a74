"""cfhip_alpha_sdf_array_device without a GPU: the export, the two structs against the header's text, every argument
error -- each returns before any device call, a NULL context last -- and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import alpha_sdf_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cfhip_alpha_sdf_array_device"
KERNELS = ("cfhip_alpha_sdf_classify_kernel", "cfhip_alpha_sdf_row_kernel", "cfhip_alpha_sdf_column_kernel",
           "cfhip_alpha_sdf_resolve_kernel")


def test_export_and_structs(hip_lib):
    from cuttlefish_amd import api, build
    from test_abi import _declared_symbols
    from test_lz4_abi import _struct_fields
    assert NAME in api.EXPORTS and NAME in _declared_symbols() and hasattr(hip_lib, NAME)
    assert hip_lib.cfhip_abi_version() == 1
    P, R = api.SdfParams, api.SdfResult
    fields = ["flags", "alpha_threshold", "spread", "scale", "channel_mask", "reserved"]
    assert ctypes.sizeof(P) == 24 and ctypes.sizeof(R) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [(n, 4*i) for i, n in enumerate(fields)]
    assert _struct_fields("cfhip_sdf_params") == [("float" if n == "alpha_threshold" else "uint32_t", n) for n in fields]
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [("inside", 0), ("saturated", 4), ("reserved", 8)]
    assert _struct_fields("cfhip_sdf_result") == [("uint32_t", "inside"), ("uint32_t", "saturated"), ("uint32_t", "reserved[2]")]
    assert api.SDF_RESULT_DTYPE.itemsize == 16 and api.SDF_RESULT_DTYPE.names == alpha_sdf_ref.FIELDS
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    flags = re.search(r"enum \{ CFHIP_SDF_WRAP_X = (\d+), CFHIP_SDF_WRAP_Y = (\d+) \};", header)
    assert tuple(int(v) for v in flags.groups()) == (api.SDF_WRAP_X, api.SDF_WRAP_Y) \
        == (alpha_sdf_ref.WRAP_X, alpha_sdf_ref.WRAP_Y) == (1, 2)
    assert "cfhip_alpha_sdf_array_device" in re.search(r"/\* Kernel-only time of the most recent.*?\*/", header, re.S).group(0)
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "alpha_sdf.h")).read()
    assert int(re.search(r"CFSD_MAX_SPREAD = (\d+);", shared).group(1)) == api.SDF_MAX_SPREAD == alpha_sdf_ref.MAX_SPREAD == 126
    assert int(re.search(r"CFSD_MAX_SIDE = (\d+);", shared).group(1)) == 32768
    assert int(re.search(r"CFSD_WG_X = (\d+);", shared).group(1)) == 64       # a wavefront is one row segment
    assert api.SDF_SCALES == alpha_sdf_ref.SCALES == (1, 2, 4, 8, 16)
    for k in KERNELS:
        assert k in build.BLOCK_KERNELS


def test_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    # host memory stands in for the surfaces: no call gets as far as touching them
    srcs = [np.zeros((8, 16, 4), np.float32) for _ in range(2)]
    dsts = [np.zeros((4, 8, 4), np.float32) for _ in range(2)]
    res = np.zeros(2*4, np.uint32)
    ok = dict(src=[a.ctypes.data for a in srcs], dst=[a.ctypes.data for a in dsts], layers=2, spt=1, dpt=1, w=16, h=8,
              sp=16*16, dp=8*16, flags=3, t=0.5, spread=5, scale=2, mask=8, reserved=0, res=res.ctypes.data, params=True)

    def call(**kw):
        a = dict(ok, **kw)
        src = (ctypes.c_void_p*len(a["src"]))(*a["src"]) if a["src"] is not None else None
        dst = (ctypes.c_void_p*len(a["dst"]))(*a["dst"]) if a["dst"] is not None else None
        p = api.SdfParams(a["flags"], a["t"], a["spread"], a["scale"], a["mask"], a["reserved"])
        return hip_lib.cfhip_alpha_sdf_array_device(None, src, a["layers"], a["spt"], a["w"], a["h"], a["sp"], dst, a["dpt"],
                                                    a["dp"], ctypes.byref(p) if a["params"] else None, a["res"], None)
    same = dict(dst=ok["src"], scale=1, dp=16*16)         # in place
    # everything right but the context: reported, and reported last
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(res=None) == api.E_INVALID and b"ctx is NULL" in err()               # the records are optional
    assert call(**same) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(t=0.0, flags=0, spread=1, mask=15) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(spread=126, scale=16, w=32768, h=16, layers=1, sp=32768*16, dp=2048*16) == api.E_INVALID and b"ctx is NULL" in err()
    for pt, comp in ((0, 1), (2, 2), (1, 4)):
        assert call(spt=pt, sp=16*4*comp + comp, dpt=pt, dp=8*4*comp + comp) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(params=False) == api.E_INVALID and b"params is NULL" in err()
    assert call(src=None) == api.E_INVALID and b"src is NULL" in err()
    assert call(dst=None) == api.E_INVALID and b"dst is NULL" in err()
    assert call(src=[srcs[0].ctypes.data, None]) == api.E_INVALID and b"src[1] is NULL" in err()
    assert call(dst=[None, dsts[1].ctypes.data]) == api.E_INVALID and b"dst[0] is NULL" in err()
    for layers in (0, 65536):
        assert call(layers=layers) == api.E_INVALID and b"layers" in err()
    for w, h in ((0, 8), (16, 0), (32770, 8), (16, 32770), (0xFFFFFFFE, 2)):
        assert call(w=w, h=h, sp=(1 << 40), dp=(1 << 40)) == api.E_INVALID and b"width and height" in err(), (w, h)
    for w, h in ((15, 8), (16, 7), (17, 9)):
        assert call(w=w, h=h, sp=17*16) == api.E_INVALID and b"multiple of the scale" in err(), (w, h)
    assert call(w=24, h=8, scale=16, sp=24*16) == api.E_INVALID and b"multiple of the scale" in err()
    for scale in (0, 3, 5, 6, 32, 0xFFFFFFFF):
        assert call(scale=scale) == api.E_INVALID and b"scale" in err() and b"1, 2, 4, 8 or 16" in err(), scale
    for spread in (0, 127, 128, 0xFFFFFFFF):
        assert call(spread=spread) == api.E_INVALID and b"spread" in err(), spread
    for t in (-0.0001, 1.0, 1.5, float("nan"), float("inf"), float("-inf")):
        assert call(t=t) == api.E_INVALID and b"alpha_threshold" in err(), t
    for flags in (4, 8, 1 | 16, 0x80000000):
        assert call(flags=flags) == api.E_INVALID and b"flags" in err(), flags
    for mask in (0, 16, 0x18, 0xFFFFFFFF):
        assert call(mask=mask) == api.E_INVALID and b"channel_mask" in err(), mask
    assert call(reserved=1) == api.E_INVALID and b"reserved" in err()
    for pt in (-1, 3, 99):
        assert call(spt=pt) == api.E_INVALID and b"src_pixel_type" in err()
        assert call(dpt=pt) == api.E_INVALID and b"dst_pixel_type" in err()
    assert call(sp=16*16 - 4) == api.E_INVALID and b"src_pitch_bytes" in err() and b"a row" in err()
    assert call(dp=8*16 - 4) == api.E_INVALID and b"dst_pitch_bytes" in err() and b"a row" in err()
    assert call(dpt=0, dp=8*4 - 1) == api.E_INVALID and b"dst_pitch_bytes" in err() and b"a row" in err()
    assert call(sp=16*16 + 2) == api.E_INVALID and b"src_pitch_bytes" in err() and b"aligned to a component" in err()
    assert call(dpt=2, dp=8*8 + 1) == api.E_INVALID and b"dst_pitch_bytes" in err() and b"aligned to a component" in err()
    assert call(src=[srcs[0].ctypes.data, srcs[1].ctypes.data + 2]) == api.E_INVALID and b"src[1] not aligned" in err()
    assert call(dpt=2, dp=8*8, dst=[dsts[0].ctypes.data + 1, dsts[1].ctypes.data]) == api.E_INVALID and b"dst[0] not aligned" in err()
    # in place needs scale 1 and one pixel type
    assert call(dst=ok["src"]) == api.E_INVALID and b"in place" in err()
    assert call(**dict(same, dpt=2, dp=16*8)) == api.E_INVALID and b"in place" in err()
    assert call(dst=[dsts[0].ctypes.data, srcs[1].ctypes.data]) == api.E_INVALID and b"dst[1] equals src[1]" in err()
    assert call(w=32768, h=32768, layers=3, sp=32768*16, dp=16384*16) == api.E_INVALID and b"2^31 texels" in err()
    assert not res.any() and not any(a.any() for a in srcs + dsts)


def test_make_sdf_params_rejects_every_bad_field():
    from cuttlefish_amd import api
    p = api.make_sdf_params(16, 8, 0.25, (False, True), "gb")
    assert (p.flags, p.alpha_threshold, p.spread, p.scale, p.channel_mask, p.reserved) == (2, 0.25, 16, 8, 6, 0)
    p = api.make_sdf_params(1)
    assert (p.flags, p.alpha_threshold, p.spread, p.scale, p.channel_mask, p.reserved) == (0, 0.5, 1, 1, 8, 0)
    assert api.make_sdf_params(126, 16, 0.0, True, "RGBA").channel_mask == 15 and api.make_sdf_params(3, wrap=True).flags == 3
    assert api.make_sdf_params(3, channels=5).channel_mask == 5
    for bad in (dict(spread=0), dict(spread=127), dict(spread=-1), dict(spread=2.5), dict(spread=True),
                dict(scale=0), dict(scale=3), dict(scale=32), dict(scale=-2), dict(scale=True),
                dict(threshold=-0.1), dict(threshold=1.0), dict(threshold=float("nan")), dict(threshold=float("inf")),
                dict(threshold=1.0 - 1e-12),                # rounds to 1.0f
                dict(channels=""), dict(channels="x"), dict(channels="aa"), dict(channels=0), dict(channels=16),
                dict(channels=None), dict(channels=True)):
        with pytest.raises(ValueError):
            api.make_sdf_params(**dict(dict(spread=4), **bad))
    with pytest.raises((ValueError, TypeError)):
        api.make_sdf_params(4, wrap=(True, False, True))


def test_python_surface():
    from cuttlefish_amd import Dimension, Image, Texture, api, plan_process_image, process_image
    for f in (api.Context.alpha_sdf_device, api.Context.alpha_sdf, Image.distance_field, Texture.alpha_distance_field,
              Texture.sdf_results, api.make_sdf_params):
        assert callable(f)
    sig = inspect.signature(api.Context.alpha_sdf_device)
    assert list(sig.parameters)[1:] == ["srcs", "pixel_type", "width", "height", "row_pitch_bytes", "dsts", "dst_pixel_type",
                                        "dst_row_pitch_bytes", "spread", "scale", "threshold", "wrap", "channels", "results",
                                        "stream"]
    assert [sig.parameters[n].default for n in ("scale", "threshold", "wrap", "channels", "results", "stream")] == \
        [1, 0.5, (False, False), "a", 0, 0]
    sig = inspect.signature(api.Context.alpha_sdf)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[3:]] == \
        [("scale", 1), ("threshold", 0.5), ("wrap", (False, False)), ("channels", "a"), ("out_dtype", None)]
    sig = inspect.signature(Image.distance_field)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[2:]] == \
        [("scale", 1), ("threshold", 0.5), ("wrap", False), ("channels", "a")]
    sig = inspect.signature(Texture.alpha_distance_field)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[2:]] == [("threshold", 0.5), ("wrap", False), ("channels", "a")]
    assert "alpha_coverage" not in sig.parameters
    # what is refused is refused before any device work
    t = Texture(Dimension.Dim3D, 4, 4, 4)
    for d in range(4):
        assert t.set_image(np.zeros((4, 4, 4), np.float32), 0, d)
    assert t.alpha_distance_field(2) is False and Texture().alpha_distance_field(2) is False and t.sdf_results() == []
    assert Image(np.zeros((2, 2, 4), np.float32), rgbf=True).distance_field(2) is None
    with pytest.raises(ValueError):
        Image(np.zeros((6, 8, 4), np.uint8)).distance_field(2, scale=4)
    with pytest.raises(ValueError):
        Image(np.zeros((8, 8, 4), np.uint8)).distance_field(127)
    # the per-image pipeline: off by default; the classes in front of the first resize, the field directly after it
    assert inspect.signature(process_image).parameters["sdf"].default is None
    assert inspect.signature(plan_process_image).parameters["sdf"].default is None
    plain = plan_process_image(8, 6, 16, 12, 1, 0)
    assert [s[0] for s in plan_process_image(8, 6, 16, 12, 1, 0, sdf=None)] == [s[0] for s in plain]
    field = plan_process_image(8, 6, 16, 12, 1, 0, sdf=dict(spread=4, threshold=0.25, wrap=(True, False), channels="ga"))
    assert [s[0] for s in plain] == ["ops", "resize"] and [s[0] for s in field] == ["ops", "sdf_class", "resize", "sdf"]
    assert field[3] == ("sdf", 4, 2, 0.25, (True, False), "ga")
    assert [s[0] for s in plan_process_image(8, 8, 8, 8, 0, 0, sdf=dict(spread=3))] == ["ops", "sdf_class", "sdf"]
    assert plan_process_image(8, 8, 8, 8, 0, 0, sdf=dict(spread=3))[2] == ("sdf", 3, 1, 0.5, (False, False), "a")
    assert [s[0] for s in plan_process_image(8, 8, 128, 128, 0, 0, flip_x=True, bleed={}, sdf=dict(spread=3))] == \
        ["bleed", "sdf_class", "resize", "sdf", "ops"]
    for w, h in ((8, 8), (5, 4), (32, 24), (1, 1)):        # 2 x 1.5, 3.2 x 3, enlarging, 16 x 12
        with pytest.raises(ValueError):
            plan_process_image(w, h, 16, 12, 0, 0, sdf=dict(spread=3))
    with pytest.raises(ValueError):
        plan_process_image(8, 8, 16, 16, 0, 0, premultiply=True, sdf=dict(spread=3))
    with pytest.raises(ValueError):
        process_image(np.zeros((4, 4, 4), np.uint8), 0, 0, 4, 4, premultiply=True, sdf=dict(spread=3))
    with pytest.raises(ValueError):
        process_image(np.zeros((12, 12, 4), np.uint8), 0, 0, 4, 4, sdf=dict(spread=3))      # a ratio of 3
    for bad in (dict(radius=3), dict(threshold=0.5), dict(spread=0), dict(spread=3, channels="q")):
        with pytest.raises(ValueError):
            plan_process_image(8, 8, 16, 16, 0, 0, sdf=bad)
