"""cfhip_alpha_bleed_array_device without a GPU: the export, the two structs against the header's text, every argument
error -- each returns before any device call, a NULL context last -- and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import alpha_bleed_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cfhip_alpha_bleed_array_device"


def test_export_and_structs(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    from test_lz4_abi import _struct_fields
    assert NAME in api.EXPORTS and NAME in _declared_symbols() and hasattr(hip_lib, NAME)
    assert hip_lib.cfhip_abi_version() == 1
    P, R = api.BleedParams, api.BleedResult
    assert ctypes.sizeof(P) == 12
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("flags", 0), ("alpha_threshold", 4), ("max_distance", 8)]
    assert _struct_fields("cfhip_bleed_params") == [("uint32_t", "flags"), ("float", "alpha_threshold"), ("uint32_t", "max_distance")]
    assert ctypes.sizeof(R) == 16 and tuple(n for n, _ in R._fields_) == alpha_bleed_ref.FIELDS
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 4, 8, 12]
    assert _struct_fields("cfhip_bleed_result") == [("uint32_t", n) for n in alpha_bleed_ref.FIELDS]
    assert api.BLEED_RESULT_DTYPE.itemsize == 16 and api.BLEED_RESULT_DTYPE.names == alpha_bleed_ref.FIELDS
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    flags = re.search(r"enum \{ CFHIP_BLEED_WRAP_X = (\d+), CFHIP_BLEED_WRAP_Y = (\d+) \};", header)
    assert tuple(int(v) for v in flags.groups()) == (api.BLEED_WRAP_X, api.BLEED_WRAP_Y) \
        == (alpha_bleed_ref.WRAP_X, alpha_bleed_ref.WRAP_Y) == (1, 2)
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "alpha_bleed.h")).read()
    assert int(re.search(r"CFAB_NONE = (0x\w+)u;", shared).group(1), 16) == alpha_bleed_ref.NONE
    assert int(re.search(r"CFAB_MAX_SIDE = (\d+);", shared).group(1)) == 32768
    # a wavefront is one row segment: 64 lanes along x
    assert int(re.search(r"CFAB_WG_X = (\d+);", shared).group(1)) == 64


def test_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    # host memory stands in for the surfaces: no call gets as far as touching them
    imgs = [np.zeros((6, 8, 4), np.float32) for _ in range(2)]
    res = np.zeros(2*4, np.uint32)
    ok = dict(images=[a.ctypes.data for a in imgs], layers=2, pt=1, w=8, h=6, pitch=8*16, flags=3, t=0.5, md=7,
              res=res.ctypes.data, params=True)

    def call(**kw):
        a = dict(ok, **kw)
        images = (ctypes.c_void_p*len(a["images"]))(*a["images"]) if a["images"] is not None else None
        params = ctypes.byref(api.BleedParams(a["flags"], a["t"], a["md"])) if a["params"] else None
        return hip_lib.cfhip_alpha_bleed_array_device(None, images, a["layers"], a["pt"], a["w"], a["h"], a["pitch"], params,
                                                      a["res"], None)
    # everything right but the context: reported, and reported last
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(res=None) == api.E_INVALID and b"ctx is NULL" in err()               # the records are optional
    assert call(t=0.0, md=0, flags=0) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(md=65535, w=32768, h=1, layers=1, pitch=32768*16) == api.E_INVALID and b"ctx is NULL" in err()
    for pt, comp in ((0, 1), (2, 2), (1, 4)):
        assert call(pt=pt, pitch=8*4*comp + comp) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(params=False) == api.E_INVALID and b"params is NULL" in err()
    assert call(images=None) == api.E_INVALID and b"images is NULL" in err()
    assert call(images=[imgs[0].ctypes.data, None]) == api.E_INVALID and b"images[1] is NULL" in err()
    assert call(layers=0) == api.E_INVALID and b"layers" in err()
    assert call(layers=65536) == api.E_INVALID and b"layers" in err()
    for w, h in ((0, 6), (8, 0), (32769, 6), (8, 32769), (0xFFFFFFFF, 1)):
        assert call(w=w, h=h, pitch=(1 << 40)) == api.E_INVALID and b"width and height" in err(), (w, h)
    for pt in (-1, 3, 99):
        assert call(pt=pt) == api.E_INVALID and b"pixel_type" in err()
    for flags in (4, 8, 1 | 16, 0x80000000):
        assert call(flags=flags) == api.E_INVALID and b"flags" in err(), flags
    for t in (-0.0001, 1.0, 1.5, float("nan"), float("inf"), float("-inf")):
        assert call(t=t) == api.E_INVALID and b"alpha_threshold" in err(), t
    for md in (65536, 0xFFFFFFFF):
        assert call(md=md) == api.E_INVALID and b"max_distance" in err()
    assert call(pitch=8*16 - 4) == api.E_INVALID and b"pitch_bytes" in err() and b"a row" in err()
    assert call(pt=0, pitch=8*4 - 1) == api.E_INVALID and b"a row" in err()
    assert call(pitch=8*16 + 2) == api.E_INVALID and b"aligned to a component" in err()
    assert call(pt=2, pitch=8*8 + 1) == api.E_INVALID and b"aligned to a component" in err()
    assert call(images=[imgs[0].ctypes.data, imgs[1].ctypes.data + 2]) == api.E_INVALID and b"images[1] not aligned" in err()
    assert call(pt=2, images=[imgs[0].ctypes.data + 1, imgs[1].ctypes.data]) == api.E_INVALID and b"images[0] not aligned" in err()
    assert call(w=32768, h=32768, layers=3, pitch=32768*16) == api.E_INVALID and b"2^31 texels" in err()
    assert not res.any() and not any(a.any() for a in imgs)


def test_python_surface():
    from cuttlefish_amd import Dimension, Image, Texture, api, plan_process_image, process_image
    for f in (api.Context.alpha_bleed_device, api.Context.alpha_bleed, Image.bleed_alpha, Texture.bleed_alpha,
              Texture.bleed_results, api.make_bleed_params):
        assert callable(f)
    sig = inspect.signature(api.Context.alpha_bleed_device)
    assert list(sig.parameters)[1:] == ["images", "pixel_type", "width", "height", "row_pitch_bytes", "threshold", "wrap",
                                        "max_distance", "results", "stream"]
    assert [sig.parameters[n].default for n in ("threshold", "wrap", "max_distance", "results", "stream")] == \
        [0.0, (False, False), 0, 0, 0]
    for f in (Image.bleed_alpha, Texture.bleed_alpha):
        sig = inspect.signature(f)
        assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [("threshold", 0.0), ("wrap", False), ("max_distance", 0)]
    p = api.make_bleed_params(0.25, (False, True), 9)
    assert (p.flags, p.alpha_threshold, p.max_distance) == (2, 0.25, 9)
    assert api.make_bleed_params(wrap=True).flags == 3 and api.make_bleed_params().flags == 0
    # what is refused is refused before any device work
    t = Texture(Dimension.Dim3D, 4, 4, 4)
    for d in range(4):
        assert t.set_image(np.zeros((4, 4, 4), np.float32), 0, d)
    assert t.bleed_alpha() is False and Texture().bleed_alpha() is False and t.bleed_results() == []
    assert Image(np.zeros((2, 2, 4), np.float32), rgbf=True).bleed_alpha() is False
    # the per-image pipeline: off by default, one step directly before the first resize, never with premultiplication
    assert inspect.signature(process_image).parameters["bleed"].default is None
    assert inspect.signature(plan_process_image).parameters["bleed"].default is None
    plain = plan_process_image(8, 8, 16, 12, 1, 0)
    bled = plan_process_image(8, 8, 16, 12, 1, 0, bleed=dict(threshold=0.5, wrap=(True, False), max_distance=4))
    assert [s[0] for s in plain] == ["ops", "resize"] and [s[0] for s in bled] == ["ops", "bleed", "resize"]
    assert bled[1] == ("bleed", 0.5, (True, False), 4)
    assert [s[0] for s in plan_process_image(8, 8, 8, 8, 0, 0, bleed={})] == ["ops", "bleed"]
    assert [s[0] for s in plan_process_image(8, 8, 16, 16, 0, 0, flip_x=True, bleed={})] == ["bleed", "resize", "ops"]
    assert [s[0] for s in plan_process_image(8, 8, 16, 16, 0, 0, bleed=None)] == ["resize"]
    with pytest.raises(ValueError):
        plan_process_image(8, 8, 16, 16, 0, 0, premultiply=True, bleed={})
    with pytest.raises(ValueError):
        process_image(np.zeros((4, 4, 4), np.uint8), 0, 0, 4, 4, premultiply=True, bleed=dict(threshold=0.5))
    with pytest.raises(ValueError):
        plan_process_image(8, 8, 16, 16, 0, 0, bleed=dict(radius=3))
