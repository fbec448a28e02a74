"""cfhip_mip_post_array_device and cfhip_alpha_coverage_device without a GPU: the exports, the two structs against the
header's text, every argument error -- each returns before any device call, a NULL context last -- and the Python
surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import mip_post_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_mip_post_array_device", "cfhip_alpha_coverage_device")


def test_exports_and_structs(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    from test_lz4_abi import _struct_fields
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    P, R = api.MipPostParams, api.MipPostResult
    assert ctypes.sizeof(P) == 8 and [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("flags", 0), ("alpha_threshold", 4)]
    assert _struct_fields("cfhip_mip_post_params") == [("uint32_t", "flags"), ("float", "alpha_threshold")]
    assert ctypes.sizeof(R) == 16 and tuple(n for n, _ in R._fields_) == mip_post_ref.FIELDS
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 4, 8, 12]
    assert _struct_fields("cfhip_mip_post_result") == [("float", "scale")] + [("uint32_t", n) for n in mip_post_ref.FIELDS[1:]]
    assert api.MIP_POST_RESULT_DTYPE.itemsize == 16 and api.MIP_POST_RESULT_DTYPE.names == mip_post_ref.FIELDS
    S = api.CoverageSurface
    assert ctypes.sizeof(S) == 32 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 12, 16, 24]
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    flags = re.search(r"enum \{ CFHIP_MIP_POST_COVERAGE = (\d+), CFHIP_MIP_POST_NORMALIZE = (\d+), "
                      r"CFHIP_MIP_POST_SIGNED_NORMALS = (\d+) \};", header)
    assert tuple(int(v) for v in flags.groups()) == (api.MIP_POST_COVERAGE, api.MIP_POST_NORMALIZE, api.MIP_POST_SIGNED_NORMALS) \
        == (mip_post_ref.COVERAGE, mip_post_ref.NORMALIZE, mip_post_ref.SIGNED_NORMALS) == (1, 2, 4)
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "mip_post.h")).read()
    one, lo, hi = (int(v, 16) for v in re.search(
        r"CFMP_BITS_ONE = (0x\w+)u, CFMP_BITS_MIN = (0x\w+)u, CFMP_BITS_MAX = (0x\w+)u", shared).groups())
    assert (one, lo, hi) == (mip_post_ref.ONE, mip_post_ref.bits(mip_post_ref.S_MIN), mip_post_ref.bits(mip_post_ref.S_MAX))
    # the search: 16-way, as many passes as take the range between 1 and a clamp down to two adjacent patterns
    passes = int(re.search(r"CFMP_SEARCH_PASSES = (\d+);", shared).group(1))
    assert 16**passes == hi - one == one - lo


def test_mip_post_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    # host memory stands in for the buffers: no call gets as far as touching them
    src = np.zeros((8, 8, 4), np.float32)
    lv = [np.zeros((4, 4, 4), np.float32), np.zeros((2, 2, 4), np.float32), np.zeros((1, 1, 4), np.float32)]
    res = np.zeros(3*4, np.uint32)
    ok = dict(srcs=[src.ctypes.data], layers=1, pt=1, w=8, h=8, pitch=8*16, levels=[a.ctypes.data for a in lv], n=4,
              flags=1, t=0.5, res=res.ctypes.data, params=True)

    def call(**kw):
        a = dict(ok, **kw)
        srcs = (ctypes.c_void_p*len(a["srcs"]))(*a["srcs"]) if a["srcs"] is not None else None
        levels = (ctypes.c_void_p*len(a["levels"]))(*a["levels"]) if a["levels"] is not None else None
        params = ctypes.byref(api.MipPostParams(a["flags"], a["t"])) if a["params"] else None
        return hip_lib.cfhip_mip_post_array_device(None, srcs, a["layers"], a["pt"], a["w"], a["h"], a["pitch"], levels, a["n"],
                                                   params, a["res"], None)
    # everything right but the context: reported, and reported last
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(flags=2, res=None) == api.E_INVALID and b"ctx is NULL" in err()      # results are ignored without COVERAGE
    assert call(flags=2, t=float("nan")) == api.E_INVALID and b"ctx is NULL" in err()  # and so is the threshold
    assert call(params=False) == api.E_INVALID and b"params is NULL" in err()
    assert call(srcs=None) == api.E_INVALID and b"srcs is NULL" in err()
    assert call(levels=None) == api.E_INVALID and b"levels is NULL" in err()
    assert call(srcs=[None]) == api.E_INVALID and b"srcs[0] is NULL" in err()
    assert call(levels=[lv[0].ctypes.data, None, lv[2].ctypes.data]) == api.E_INVALID and b"levels[1]" in err() and b"NULL" in err()
    assert call(layers=0) == api.E_INVALID and b"layers" in err()
    for flags in (0, 8, 1 | 16, 0x80000000):
        assert call(flags=flags) == api.E_INVALID and b"flags" in err(), flags
    for flags in (4, 1 | 4):
        assert call(flags=flags) == api.E_INVALID and b"SIGNED_NORMALS without NORMALIZE" in err()
    for t in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        for flags in (1, 1 | 2, 1 | 2 | 4):
            assert call(t=t, flags=flags) == api.E_INVALID and b"alpha_threshold" in err(), t
    for n in (0, 1):
        assert call(n=n) == api.E_INVALID and b"levels_count" in err()
    assert call(n=5) == api.E_INVALID and b"levels_count" in err()                  # an 8 x 8 chain has 4 levels
    assert call(w=1, h=1, pitch=16, n=2) == api.E_INVALID and b"levels_count" in err()   # a 1 x 1 chain has nothing to repair
    assert call(pitch=8*16 - 1) == api.E_INVALID and b"src_pitch_bytes" in err()
    assert call(pt=0, pitch=8*4 - 1) == api.E_INVALID and b"src_pitch_bytes" in err()
    assert call(res=None) == api.E_INVALID and b"results_device" in err()
    assert call(w=0) == api.E_INVALID and b"zero width or height" in err()
    assert call(h=0) == api.E_INVALID and b"zero width or height" in err()
    assert call(pt=3) == api.E_INVALID and b"src_pixel_type" in err()
    assert call(levels=[lv[0].ctypes.data + 4] + ok["levels"][1:]) == api.E_INVALID and b"aligned" in err()
    assert call(w=1 << 16, h=1 << 15, pitch=(1 << 16)*16) == api.E_INVALID and b"2^30" in err()
    assert not res.any() and not any(a.any() for a in lv)


def test_alpha_coverage_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: hip_lib.cfhip_last_error(None)          # noqa: E731
    img = np.zeros((3, 5, 4), np.float32)
    counts = np.zeros(2, np.uint32)
    ok = dict(pixels=img.ctypes.data, pt=1, w=5, h=3, pitch=5*16, n=1, t=0.5, s=1.0, counts=counts.ctypes.data, surfaces=True)

    def call(**kw):
        a = dict(ok, **kw)
        surf = (api.CoverageSurface*1)()
        surf[0].pixels, surf[0].pixel_type, surf[0].width, surf[0].height = a["pixels"], a["pt"], a["w"], a["h"]
        surf[0].pitch_bytes = a["pitch"]
        return hip_lib.cfhip_alpha_coverage_device(None, surf if a["surfaces"] else None, a["n"], a["t"], a["s"], a["counts"], None)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(surfaces=False) == api.E_INVALID and b"surfaces is NULL" in err()
    assert call(counts=None) == api.E_INVALID and b"counts_device is NULL" in err()
    assert call(n=0) == api.E_INVALID and b"count is 0" in err()
    assert call(pixels=None) == api.E_INVALID and b"pixels is NULL" in err()
    for t in (0.0, -1.0, 1.5, float("nan")):
        assert call(t=t) == api.E_INVALID and b"threshold" in err()
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert call(s=s) == api.E_INVALID and b"scale" in err()
    assert call(w=0) == api.E_INVALID and b"zero width or height" in err()
    assert call(h=0) == api.E_INVALID and b"zero width or height" in err()
    assert call(pt=-1) == api.E_INVALID and b"pixel type" in err()
    assert call(pitch=5*16 - 4) == api.E_INVALID and b"pitch_bytes" in err()
    assert call(pt=2, pitch=5*8 + 1) == api.E_INVALID and b"aligned" in err()
    assert call(pixels=img.ctypes.data + 2) == api.E_INVALID and b"aligned" in err()
    assert not counts.any()


def test_python_surface():
    from cuttlefish_amd import Dimension, Texture, api
    for f in (api.Context.mip_post_device, api.Context.alpha_coverage_device, api.Context.alpha_coverage,
              Texture.mip_post_results, api.make_mip_post_params):
        assert callable(f)
    p = api.make_mip_post_params(0.25, "snorm")
    assert (p.flags, p.alpha_threshold) == (7, 0.25)
    assert api.make_mip_post_params(None, "unorm").flags == 2 and api.make_mip_post_params(1.0).flags == 1
    with pytest.raises(ValueError):
        api.make_mip_post_params(0.5, "float")
    assert "straight alpha" in api.Context.mip_post_device.__doc__ and "straight alpha" in Texture.generate_mipmaps.__doc__
    # what is refused is refused before any device work: a volume, an unknown storage, a threshold outside (0, 1]
    t = Texture(Dimension.Dim3D, 4, 4, 4)
    for d in range(4):
        assert t.set_image(np.zeros((4, 4, 4), np.float32), 0, d)
    assert t.generate_mipmaps(alpha_coverage=0.5) is False and t.generate_mipmaps(normalize="unorm") is False
    t = Texture(4, 4)
    assert t.set_image(np.zeros((4, 4, 4), np.float32))
    assert t.generate_mipmaps(normalize="float") is False and t.generate_mipmaps(alpha_coverage=0.0) is False
    assert t.generate_mipmaps(alpha_coverage=1.5) is False and t.mip_post_results() == []
