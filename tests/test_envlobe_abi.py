"""The lobe tables, the BRDF lookup table and the irradiance cube without a GPU: the exports, the struct and the constants
against the header's text, every argument error -- each returns before any device call, a NULL context last -- the C table
helpers against the numpy ones, and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import envlobe_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_lobe_sample_table", "cfhip_hammersley_table", "cfhip_brdf_lut_device", "cfhip_cube_irradiance_device")
HOST_ONLY = NAMES[:2]
KERNELS = ("cfhip_brdf_lut_kernel", "cfhip_cube_irradiance_kernel")


def test_exports_struct_and_constants(hip_lib):
    from cuttlefish_amd import api, build
    from test_abi import _declared_symbols
    from test_lz4_abi import _struct_fields
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    H = api.HammersleySample
    assert ctypes.sizeof(H) == 16
    assert [(n, getattr(H, n).offset) for n, _ in H._fields_] == [("cos_phi", 0), ("sin_phi", 4), ("xi1", 8), ("reserved", 12)]
    assert _struct_fields("cfhip_hammersley_sample") == [("float", n) for n in ("cos_phi", "sin_phi", "xi1", "reserved")]
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    timed = re.search(r"/\* Kernel-only time of the most recent.*?\*/", header, re.S).group(0)
    for n in NAMES:
        assert (n in timed) == (n not in HOST_ONLY), n
    lobes = re.search(r"enum \{ CFHIP_LOBE_GGX = (\d), CFHIP_LOBE_CHARLIE = (\d), CFHIP_LOBE_LAMBERT = (\d) \};", header)
    assert tuple(int(g) for g in lobes.groups()) == (api.LOBE_GGX, api.LOBE_CHARLIE, api.LOBE_LAMBERT) \
        == (E.LOBE_GGX, E.LOBE_CHARLIE, E.LOBE_LAMBERT) == (0, 1, 2)
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "envmap.h")).read()
    assert int(re.search(r"CFENV_MAX_LUT = (\d+);", shared).group(1)) == api.ENV_MAX_LUT == E.MAX_LUT == 1024
    assert re.search(r"CFENV_LOBE_GGX = 0, CFENV_LOBE_CHARLIE = 1, CFENV_LOBE_LAMBERT = 2;", shared)
    for k in KERNELS:
        assert k in build.BLOCK_KERNELS


def _err(hip_lib):
    return hip_lib.cfhip_last_error(None)


def test_brdf_lut_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: _err(hip_lib)                            # noqa: E731
    # host memory stands in for the surface: no call gets as far as touching it
    dst = np.full((3, 5, 4), 7.0, np.float32)
    table = E.hammersley_table(64)
    ok = dict(dst=dst.ctypes.data, w=5, h=3, table=table, S=64, sheen=0)

    def call(**kw):
        a = dict(ok, **kw)
        t = None if a["table"] is None else np.ascontiguousarray(a["table"], np.float32)
        return hip_lib.cfhip_brdf_lut_device(None, a["dst"], a["w"], a["h"], None if t is None else t.ctypes.data, a["S"],
                                             a["sheen"], None)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(sheen=1, w=1, h=1) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(table=E.hammersley_table(4096), S=4096) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(dst=None) == api.E_INVALID and b"dst is NULL" in err()
    assert call(dst=dst.ctypes.data + 4) == api.E_INVALID and b"dst not aligned" in err()
    for w, h in ((0, 3), (5, 0), (1025, 3), (5, 1025)):
        assert call(w=w, h=h) == api.E_INVALID and b"width and height are 1 to 1024" in err(), (w, h)
    assert call(table=None) == api.E_INVALID and b"table is NULL" in err()
    for S in (0, 32, 100, 4160, 8192):
        assert call(S=S) == api.E_INVALID and b"samples is" in err(), S
    assert call(sheen=2) == api.E_INVALID and b"sheen is 0 or 1" in err()
    for field, value in ((0, np.nan), (1, np.inf), (2, 0.0), (2, 1.0), (2, -0.5), (2, np.nan)):
        bad = table.copy()
        bad[9, field] = value
        assert call(table=bad) == api.E_INVALID and b"table[9]" in err(), (field, value)
    assert (dst == 7.0).all()


def test_cube_irradiance_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: _err(hip_lib)                            # noqa: E731
    faces = [np.full((2, 2, 4), 7.0, np.float32) for _ in range(6)]
    rec = np.zeros(37, np.float64)
    ok = dict(rec=rec.ctypes.data, faces=[a.ctypes.data for a in faces], n=2, over_pi=0)

    def call(**kw):
        a = dict(ok, **kw)
        arr = (ctypes.c_void_p*6)(*a["faces"]) if a["faces"] is not None else None
        return hip_lib.cfhip_cube_irradiance_device(None, a["rec"], arr, a["n"], a["over_pi"], None)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(over_pi=1, n=8192) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(rec=None) == api.E_INVALID and b"sh9_result_device is NULL" in err()
    assert call(rec=rec.ctypes.data + 4) == api.E_INVALID and b"sh9_result_device not aligned" in err()
    assert call(faces=None) == api.E_INVALID and b"faces is NULL" in err()
    for n in (0, 8193):
        assert call(n=n) == api.E_INVALID and b"face_size" in err()
    assert call(faces=ok["faces"][:4] + [None] + ok["faces"][5:]) == api.E_INVALID and b"faces[4] is NULL" in err()
    assert call(faces=[ok["faces"][0] + 8] + ok["faces"][1:]) == api.E_INVALID and b"faces[0] not aligned" in err()
    assert call(faces=ok["faces"][:5] + [rec.ctypes.data]) == api.E_INVALID and b"faces[5] equals sh9_result_device" in err()
    assert call(over_pi=2) == api.E_INVALID and b"over_pi is 0 or 1" in err()
    assert all((a == 7.0).all() for a in faces) and not rec.any()


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("roughness", [0.3, 0.5, 1.0])
def test_the_c_lobe_tables_are_the_numpy_ones_within_one_unit_in_the_last_place(hip_lib, kind, roughness):
    """the two call different pow, cos, sin and log2: every field within one float32 unit in the last place"""
    from cuttlefish_amd import api
    for samples, n, levels in ((64, 256, 9), (256, 16, 5), (1088, 5, 1)):
        got = api.lobe_sample_table(kind, roughness, samples, n, levels)
        want = E.lobe_sample_table(kind, roughness, samples, n, levels)
        assert got.shape == want.shape == (samples, 4) and got.dtype == want.dtype == np.float32
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        assert ((got[:, 2] == 0) == (want[:, 2] == 0)).all() and (got[want[:, 2] == 0, 3] == 0).all()
        if kind == api.LOBE_GGX:
            assert got.tobytes() == api.ggx_sample_table(roughness, samples, n, levels).tobytes()
        if kind == api.LOBE_LAMBERT:
            assert (got[:, 2] == want[:, 2]).all()         # lz has no library call in it


@pytest.mark.parametrize("samples", [64, 192, 1088, 4096])
def test_the_c_hammersley_table_is_the_numpy_one_within_one_unit_in_the_last_place(hip_lib, samples):
    from cuttlefish_amd import api
    got, want = api.hammersley_table(samples), E.hammersley_table(samples)
    assert got.shape == want.shape == (samples, 4) and got.dtype == np.float32
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert got[:, 2:].tobytes() == want[:, 2:].tobytes()   # xi1 and the reserved 0 have no library call in them


def test_the_c_table_helpers_refuse_what_has_no_table(hip_lib):
    from cuttlefish_amd import api
    out = np.full((64, 4), 7.0, np.float32)
    p = out.ctypes.data_as(ctypes.POINTER(api.GgxSample))
    for kind, r, s, n, levels in ((3, 0.5, 64, 16, 5), (-1, 0.5, 64, 16, 5), (0, 0.0, 64, 16, 5), (1, 0.0, 64, 16, 5),
                                  (1, 1.5, 64, 16, 5), (1, float("nan"), 64, 16, 5), (1, 0.5, 32, 16, 5), (2, 0.5, 0, 16, 5),
                                  (2, 0.5, 100, 16, 5), (2, 0.5, 8192, 16, 5), (2, 0.5, 64, 0, 1), (1, 0.5, 64, 8193, 1),
                                  (2, 0.5, 64, 16, 0), (1, 0.5, 64, 16, 6)):
        assert hip_lib.cfhip_lobe_sample_table(kind, r, s, n, levels, p) == api.E_INVALID, (kind, r, s, n, levels)
    for kind in (0, 1, 2):
        assert hip_lib.cfhip_lobe_sample_table(kind, 0.5, 64, 16, 5, None) == api.E_INVALID
    hp = out.ctypes.data_as(ctypes.POINTER(api.HammersleySample))
    for s in (0, 32, 100, 8192):
        assert hip_lib.cfhip_hammersley_table(s, hp) == api.E_INVALID
    assert hip_lib.cfhip_hammersley_table(64, None) == api.E_INVALID
    assert (out == 7.0).all()
    # Lambert reads no roughness: any value, the same table
    assert hip_lib.cfhip_lobe_sample_table(2, float("nan"), 64, 16, 5, p) == 0 and not (out == 7.0).any()
    assert out.tobytes() == api.lobe_sample_table(api.LOBE_LAMBERT, 0.9, 64, 16, 5).tobytes()
    assert hip_lib.cfhip_hammersley_table(64, hp) == 0 and out.tobytes() == api.hammersley_table(64).tobytes()
    for bad in (dict(kind=3), dict(kind=True), dict(kind=1, roughness=0.0), dict(kind=0, roughness=2.0), dict(samples=100),
                dict(samples=True), dict(samples=64.0), dict(face_size=0), dict(source_levels=9)):
        with pytest.raises(ValueError):
            api.lobe_sample_table(**dict(dict(kind=2, roughness=0.5, samples=64, face_size=16, source_levels=5), **bad))
    for bad in (0, 100, True, 64.0, 8192):
        with pytest.raises(ValueError):
            api.hammersley_table(bad)


def test_python_surface():
    from cuttlefish_amd import CubeFace, Dimension, Texture, api
    C = api.Context
    for f in (C.brdf_lut_device, C.brdf_lut, C.cube_irradiance_device, C.cube_irradiance, C.cube_prefilter_lobe,
              api.lobe_sample_table, api.hammersley_table, Texture.brdf_lut, Texture.prefilter_lobe, Texture.irradiance_cube):
        assert callable(f)

    def params(f, skip=1):
        return [(n, p.default) for n, p in list(inspect.signature(f).parameters.items())[skip:]]
    X = inspect.Parameter.empty
    assert params(C.brdf_lut_device) == [("dst", X), ("width", X), ("height", X), ("table", X), ("sheen", False), ("stream", 0)]
    assert params(C.brdf_lut) == [("width", X), ("height", X), ("samples", 1024), ("sheen", False)]
    assert params(C.cube_irradiance_device) == [("sh9_result", X), ("faces", X), ("face_size", X), ("over_pi", False), ("stream", 0)]
    assert params(C.cube_irradiance) == [("coeffs", X), ("face_size", X), ("over_pi", False)]
    assert params(C.cube_prefilter_lobe) == [("faces", X), ("kind", X), ("roughness", X), ("samples", 256)]
    assert params(api.lobe_sample_table, 0) == [("kind", X), ("roughness", X), ("samples", X), ("face_size", X), ("source_levels", X)]
    assert params(api.hammersley_table, 0) == [("samples", X)]
    assert params(Texture.brdf_lut, 0) == [("size", 128), ("samples", 1024), ("sheen", False), ("device_id", 0)]
    assert params(Texture.prefilter_lobe) == [("kind", X), ("mip_levels", None), ("samples", 256), ("roughness", None)]
    assert params(Texture.irradiance_cube) == [("face_size", 32), ("method", "sh9"), ("samples", 1024)]
    # what is no complete cube is refused before any device work, as prefilter_environment refuses it
    flat = Texture(8, 8)
    assert flat.set_image(np.zeros((8, 8, 4), np.float32))
    cube = Texture(Dimension.Cube, 8, 8)
    assert cube.set_image(np.zeros((8, 8, 4), np.float32), CubeFace.PosX)
    array = Texture(Dimension.Cube, 8, 8, 2)
    for t in (Texture(), flat, cube, array):
        assert t.prefilter_lobe(api.LOBE_CHARLIE) is False and t.irradiance_cube() is None
    full = Texture(Dimension.Cube, 8, 8)
    for f in range(6):
        assert full.set_image(np.zeros((8, 8, 4), np.float32), CubeFace(f))
    assert full.prefilter_lobe(7) is False and full.prefilter_lobe(api.LOBE_CHARLIE, roughness=[0.5]) is False
    assert full.prefilter_lobe(api.LOBE_CHARLIE, mip_levels=2, roughness=[0.0, 1.5]) is False
    assert full.irradiance_cube(method="cosine") is None and full.irradiance_cube(0) is None
    assert full.irradiance_cube(3, method="lambert") is None and full.irradiance_cube(16, method="lambert") is None
    for size in (0, 1025, True, 64.0):
        assert Texture.brdf_lut(size) is None
