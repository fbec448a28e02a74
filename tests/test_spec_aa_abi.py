"""cfhip_spec_aa_array_device without a GPU: the export, the two structs against the header's text, the flags in header,
api and twin, every argument error -- each returns before any device call, a NULL context last -- and the Python
surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import spec_aa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cfhip_spec_aa_array_device"
KERNELS = ("cfhip_spec_aa_texel_kernel", "cfhip_spec_aa_moment_kernel")


def test_export_and_structs(hip_lib):
    from cuttlefish_amd import api, build
    from test_abi import _declared_symbols
    from test_lz4_abi import _struct_fields
    assert NAME in api.EXPORTS and NAME in _declared_symbols() and hasattr(hip_lib, NAME)
    assert hip_lib.cfhip_abi_version() == 1
    P, R = api.SpecAaParams, api.SpecAaResult
    fields = [("uint32_t", "struct_size"), ("uint32_t", "flags"), ("uint32_t", "channel"), ("float", "base_roughness"),
              ("float", "variance_scale"), ("float", "max_variance"), ("uint32_t", "reserved[2]")]
    assert ctypes.sizeof(P) == 32 and ctypes.sizeof(R) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [(n.split("[")[0], 4*i) for i, (_, n) in enumerate(fields)]
    assert _struct_fields("cfhip_spec_aa_params") == fields
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [(n, 4*i) for i, n in enumerate(spec_aa_ref.FIELDS)]
    assert _struct_fields("cfhip_spec_aa_result") == [("uint32_t", n) for n in spec_aa_ref.FIELDS]
    assert api.SPEC_AA_RESULT_DTYPE.itemsize == 16 and api.SPEC_AA_RESULT_DTYPE.names == spec_aa_ref.FIELDS
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    flags = re.search(r"enum \{ CFHIP_SPEC_AA_PERCEPTUAL = (\d+), CFHIP_SPEC_AA_SIGNED_NORMALS = (\d+), "
                      r"CFHIP_SPEC_AA_RECONSTRUCT_Z = (\d+) \};", header)
    assert tuple(int(v) for v in flags.groups()) \
        == (api.SPEC_AA_PERCEPTUAL, api.SPEC_AA_SIGNED_NORMALS, api.SPEC_AA_RECONSTRUCT_Z) \
        == (spec_aa_ref.PERCEPTUAL, spec_aa_ref.SIGNED_NORMALS, spec_aa_ref.RECONSTRUCT_Z) == (1, 2, 4)
    assert NAME in re.search(r"/\* Kernel-only time of the most recent.*?\*/", header, re.S).group(0)
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "spec_aa.h")).read()
    assert int(re.search(r"CFSA_MAX_SIDE = (\d+);", shared).group(1)) == spec_aa_ref.MAX_SIDE == 32768
    assert int(re.search(r"CFSA_STAGE_LEVELS = (\d+);", shared).group(1)) == 5
    assert int(re.search(r"CFSA_MAX_STAGES = (\d+);", shared).group(1)) == 3       # 15 generated levels of 32768
    assert "at most 3" in header[header.index("Specular anti-aliasing"):header.index("cfhip_spec_aa_params;")]
    for k in KERNELS:
        assert k in build.BLOCK_KERNELS


def test_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    # host memory stands in for the surfaces: no call gets as far as touching them
    W, H = 16, 8
    nrm = [np.zeros((H, W, 4), np.float32) for _ in range(2)]
    rgh = [np.zeros((H, W, 4), np.float32) for _ in range(2)]
    lev = [[np.zeros((max(1, H >> k), max(1, W >> k), 4), np.float32) for k in range(1, 5)] for _ in range(2)]
    res = np.zeros(2*4*4, np.uint32)
    ok = dict(normals=[a.ctypes.data for a in nrm], rough=[a.ctypes.data for a in rgh],
              levels=[a.ctypes.data for l in lev for a in l], layers=2, npt=1, rpt=1, w=W, h=H, np_=W*16, rp=W*16, count=5,
              size=32, flags=7, channel=1, base=0.5, scale=1.0, maxv=1.0, reserved=(0, 0), res=res.ctypes.data, params=True)

    def call(**kw):
        a = dict(ok, **kw)
        arr = lambda v: (ctypes.c_void_p*len(v))(*v) if v is not None else None      # noqa: E731
        p = api.SpecAaParams(a["size"], a["flags"], a["channel"], a["base"], a["scale"], a["maxv"],
                             (ctypes.c_uint32*2)(*a["reserved"]))
        return hip_lib.cfhip_spec_aa_array_device(None, arr(a["normals"]), a["layers"], a["npt"], a["w"], a["h"], a["np_"],
                                                  arr(a["rough"]), a["rpt"], a["rp"], arr(a["levels"]), a["count"],
                                                  ctypes.byref(p) if a["params"] else None, a["res"], None)
    # everything right but the context: reported, and reported last
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(res=None) == api.E_INVALID and b"ctx is NULL" in err()               # the records are optional
    assert call(rough=None, rpt=99, rp=0) == api.E_INVALID and b"ctx is NULL" in err()   # so is the roughness map
    assert call(rough=ok["normals"]) == api.E_INVALID and b"ctx is NULL" in err()    # which may be the normal map
    assert call(count=2, flags=0, channel=3, base=0.0, scale=0.0, maxv=0.0) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(base=1.0, scale=2.0, maxv=0.18, channel=0) == api.E_INVALID and b"ctx is NULL" in err()
    for pt, texel in ((0, 4), (2, 8), (1, 16)):
        assert call(npt=pt, np_=W*texel + texel, rpt=pt, rp=W*texel + texel//4) == api.E_INVALID and b"ctx is NULL" in err()
    big = [nrm[0].ctypes.data]*15
    assert call(w=32768, h=32768, layers=1, np_=32768*16, rp=32768*16, count=16, levels=big) == api.E_INVALID \
        and b"ctx is NULL" in err()
    assert call(params=False) == api.E_INVALID and b"params is NULL" in err()
    for size in (0, 24, 28, 36, 64):
        assert call(size=size) == api.E_INVALID and b"struct_size" in err(), size
    assert call(normals=None) == api.E_INVALID and b"normals is NULL" in err()
    assert call(levels=None) == api.E_INVALID and b"levels is NULL" in err()
    assert call(normals=[nrm[0].ctypes.data, None]) == api.E_INVALID and b"normals[1] is NULL" in err()
    assert call(rough=[None, rgh[1].ctypes.data]) == api.E_INVALID and b"rough0[0] is NULL" in err()
    assert call(levels=ok["levels"][:5] + [None] + ok["levels"][6:]) == api.E_INVALID and b"levels[5] (layer 1, level 2) is NULL" in err()
    for layers in (0, 65536):
        assert call(layers=layers) == api.E_INVALID and b"layers" in err()
    for w, h in ((0, 8), (16, 0), (32769, 8), (16, 32769), (0xFFFFFFFE, 2)):
        assert call(w=w, h=h, np_=(1 << 40), rp=(1 << 40)) == api.E_INVALID and b"width and height" in err(), (w, h)
    for flags in (8, 16, 1 | 32, 0x80000000):
        assert call(flags=flags) == api.E_INVALID and b"flags" in err(), flags
    for channel in (4, 5, 0xFFFFFFFF):
        assert call(channel=channel) == api.E_INVALID and b"channel" in err(), channel
    for base in (-0.001, 1.001, float("nan"), float("inf"), float("-inf")):
        assert call(base=base) == api.E_INVALID and b"base_roughness" in err(), base
    for bad in (-0.5, float("nan"), float("inf"), float("-inf")):
        assert call(scale=bad) == api.E_INVALID and b"variance_scale" in err(), bad
        assert call(maxv=bad) == api.E_INVALID and b"max_variance" in err(), bad
    for reserved in ((1, 0), (0, 1)):
        assert call(reserved=reserved) == api.E_INVALID and b"reserved" in err()
    for count in (0, 1, 6, 17, 0xFFFFFFFF):                # 16 x 8 has 5 levels
        assert call(count=count) == api.E_INVALID and b"levels_count" in err(), count
    for pt in (-1, 3, 99):
        assert call(npt=pt) == api.E_INVALID and b"normal_pixel_type" in err()
        assert call(rpt=pt) == api.E_INVALID and b"rough_pixel_type" in err()
    assert call(np_=W*16 - 16) == api.E_INVALID and b"normal_pitch_bytes" in err() and b"a row" in err()
    assert call(rp=W*16 - 4) == api.E_INVALID and b"rough_pitch_bytes" in err() and b"a row" in err()
    assert call(np_=W*16 + 4) == api.E_INVALID and b"normal_pitch_bytes" in err() and b"aligned to a texel" in err()
    assert call(npt=0, np_=W*4 + 2) == api.E_INVALID and b"normal_pitch_bytes" in err() and b"aligned to a texel" in err()
    assert call(rp=W*16 + 2) == api.E_INVALID and b"rough_pitch_bytes" in err() and b"aligned to a component" in err()
    assert call(normals=[nrm[0].ctypes.data, nrm[1].ctypes.data + 4]) == api.E_INVALID and b"normals[1] not aligned" in err()
    assert call(rough=[rgh[0].ctypes.data + 2, rgh[1].ctypes.data]) == api.E_INVALID and b"rough0[0] not aligned" in err()
    assert call(levels=[ok["levels"][0] + 4] + ok["levels"][1:]) == api.E_INVALID and b"levels[0] is not aligned" in err()
    assert call(w=32768, h=32769 - 1, layers=1, np_=32768*16, rp=32768*16, count=17) == api.E_INVALID and b"levels_count" in err()
    assert not res.any() and not any(a.any() for a in nrm + rgh + [x for l in lev for x in l])


def test_make_spec_aa_params_rejects_every_bad_field():
    from cuttlefish_amd import api
    p = api.make_spec_aa_params("g")
    assert (p.struct_size, p.flags, p.channel, p.base_roughness, p.variance_scale, p.max_variance, list(p.reserved)) == \
        (32, 1, 1, 0.5, 1.0, 1.0, [0, 0])
    p = api.make_spec_aa_params("A", False, True, True, 1.0, 2.0, 0.18)
    assert (p.flags, p.channel, p.base_roughness, p.variance_scale) == (6, 3, 1.0, 2.0)
    assert p.max_variance == float(np.float32(0.18))
    assert [api.make_spec_aa_params(c).channel for c in ("r", "g", "b", "a", 0, 1, 2, 3)] == [0, 1, 2, 3]*2
    for bad in (dict(channel="x"), dict(channel="rg"), dict(channel=""), dict(channel=4), dict(channel=-1),
                dict(channel=None), dict(channel=True), dict(channel=1.0),
                dict(base_roughness=-0.1), dict(base_roughness=1.1), dict(base_roughness=float("nan")),
                dict(variance_scale=-1.0), dict(variance_scale=float("inf")), dict(variance_scale=float("nan")),
                dict(variance_scale=1e39),                  # not finite as a float32
                dict(max_variance=-1.0), dict(max_variance=float("inf")), dict(max_variance=float("nan"))):
        with pytest.raises(ValueError):
            api.make_spec_aa_params(**dict(dict(channel="g"), **bad))


def test_python_surface():
    from cuttlefish_amd import Dimension, Texture, api
    for f in (api.Context.specular_aa_device, api.Context.specular_aa, Texture.specular_antialias,
              Texture.specular_aa_results, api.make_spec_aa_params):
        assert callable(f)
    sig = inspect.signature(api.Context.specular_aa_device)
    assert list(sig.parameters)[1:] == ["normals", "pixel_type", "width", "height", "pitch", "levels", "rough0",
                                        "rough_pixel_type", "rough_pitch", "channel", "perceptual", "signed_normals",
                                        "reconstruct_z", "base_roughness", "variance_scale", "max_variance", "results",
                                        "stream"]
    kw = {n: p.default for n, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY}
    assert kw == dict(rough0=None, rough_pixel_type=None, rough_pitch=0, channel=inspect.Parameter.empty, perceptual=True,
                      signed_normals=False, reconstruct_z=False, base_roughness=0.5, variance_scale=1.0, max_variance=1.0,
                      results=0, stream=0)
    sig = inspect.signature(api.Context.specular_aa)
    assert list(sig.parameters)[1:4] == ["normals", "roughness0", "levels_count"]
    sig = inspect.signature(Texture.specular_antialias)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[2:]] == \
        [("channel", "g"), ("perceptual", True), ("signed_normals", False), ("reconstruct_z", False),
         ("variance_scale", 1.0), ("max_variance", 1.0)]
    # the docstrings say what the written value is
    for f in (api.Context.specular_aa_device, Texture.specular_antialias):
        assert "not a correction" in " ".join(f.__doc__.split())
    # what is refused is refused before any device work
    img = np.zeros((4, 4, 4), np.float32)

    def tex(dim=Dimension.Dim2D, w=4, h=4, depth=0, mips=3):
        t = Texture(dim, w, h, depth, mips)
        for m in range(t.mip_level_count()):
            for d in range(max(t.depth(m), 1)):
                assert t.set_image(np.zeros((max(h >> m, 1), max(w >> m, 1), 4), np.float32), m, d)
        return t
    good = tex()
    assert Texture().specular_antialias(good) is False and good.specular_antialias(Texture()) is False
    assert good.specular_antialias(img) is False and good.specular_aa_results() == []
    assert tex(Dimension.Dim3D, depth=4).specular_antialias(good) is False                 # 3-D
    assert good.specular_antialias(tex(w=8, h=8)) is False and good.specular_antialias(tex(w=4, h=8)) is False
    assert good.specular_antialias(tex(depth=2)) is False                # another depth
    assert tex(mips=1).specular_antialias(tex(mips=1)) is False                            # fewer than 2 levels
    missing = Texture(Dimension.Dim2D, 4, 4, 0, 3)
    assert missing.set_image(img, 0) and missing.specular_antialias(good) is False        # a level is not set
    with pytest.raises(ValueError):
        good.specular_antialias(good, channel="q")
    with pytest.raises(ValueError):
        good.specular_antialias(good, max_variance=-1.0)
