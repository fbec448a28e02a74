"""The environment-map entries without a GPU: the exports, the two structs against the header's text, the constants
against csrc/envmap.h, every argument error -- each returns before any device call, a NULL context last -- the C table
helper against the numpy one, and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import envmap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cfhip_equirect_to_cube_device", "cfhip_ggx_sample_table", "cfhip_cube_prefilter_device", "cfhip_cube_sh9_device")
KERNELS = ("cfhip_equirect_to_cube_kernel", "cfhip_cube_prefilter_kernel", "cfhip_cube_copy_kernel",
           "cfhip_cube_sh9_rows_kernel", "cfhip_cube_sh9_final_kernel")


def test_exports_structs_and_constants(hip_lib):
    from cuttlefish_amd import api, build
    from test_abi import _declared_symbols
    from test_lz4_abi import _struct_fields
    for n in NAMES:
        assert n in api.EXPORTS and n in _declared_symbols() and hasattr(hip_lib, n), n
    assert hip_lib.cfhip_abi_version() == 1
    G, S = api.GgxSample, api.Sh9Result
    assert ctypes.sizeof(G) == 16 and ctypes.sizeof(S) == 37*8
    assert [(n, getattr(G, n).offset) for n, _ in G._fields_] == [("lx", 0), ("ly", 4), ("lz", 8), ("lod", 12)]
    assert _struct_fields("cfhip_ggx_sample") == [("float", n) for n in ("lx", "ly", "lz", "lod")]
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("coeff", 0), ("solid_angle", 36*8)]
    assert _struct_fields("cfhip_sh9_result") == [("double", "coeff[9][4]"), ("double", "solid_angle")]
    header = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    timed = re.search(r"/\* Kernel-only time of the most recent.*?\*/", header, re.S).group(0)
    for n in NAMES:
        assert (n in timed) == (n != "cfhip_ggx_sample_table"), n
    for quoted in ("0.282095", "0.488603", "1.092548", "0.315392", "0.546274"):
        assert quoted in header
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "envmap.h")).read()

    def const(name):
        return re.search(r"%s = ([0-9.]+);" % name, shared).group(1)
    assert int(const("CFENV_MAX_FACE")) == api.ENV_MAX_FACE == envmap_ref.MAX_FACE == 8192
    assert int(const("CFENV_MAX_PANORAMA")) == api.ENV_MAX_PANORAMA == envmap_ref.MAX_PANORAMA == 32768
    assert (int(const("CFENV_MIN_SAMPLES")), int(const("CFENV_MAX_SAMPLES"))) == (api.ENV_MIN_SAMPLES, api.ENV_MAX_SAMPLES) \
        == (envmap_ref.MIN_SAMPLES, envmap_ref.MAX_SAMPLES) == (64, 4096)
    assert int(const("CFENV_MAX_LEVELS")) == api.cube_level_count(8192) == 14
    assert int(const("CFENV_WG_X")) == 64 and int(const("CFENV_SH_VALUES")) == 37
    assert float(const("CFENV_PI")) == envmap_ref.PI == np.pi
    for name, six in (("SH_C0", "0.282095"), ("SH_C1", "0.488603"), ("SH_C2", "1.092548"), ("SH_C20", "0.315392"),
                      ("SH_C22", "0.546274")):
        v = float(const("CFENV_" + name))
        assert v == getattr(envmap_ref, name) == getattr(api, name) and "%.6f" % v == six
    assert api.ENV_SUPERSAMPLES == envmap_ref.SUPERSAMPLES == (1, 2, 4)
    for k in KERNELS:
        assert k in build.BLOCK_KERNELS


def _err(hip_lib):
    return hip_lib.cfhip_last_error(None)


def test_equirect_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: _err(hip_lib)                            # noqa: E731
    # host memory stands in for the surfaces: no call gets as far as touching them
    pano = np.zeros((4, 8, 4), np.float32)
    faces = [np.zeros((2, 2, 4), np.float32) for _ in range(6)]
    ok = dict(src=pano.ctypes.data, pt=1, w=8, h=4, pitch=8*16, faces=[a.ctypes.data for a in faces], n=2, q=2)

    def call(**kw):
        a = dict(ok, **kw)
        arr = (ctypes.c_void_p*6)(*a["faces"]) if a["faces"] is not None else None
        return hip_lib.cfhip_equirect_to_cube_device(None, a["src"], a["pt"], a["w"], a["h"], a["pitch"], arr, a["n"], a["q"], None)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    for q in (1, 4):
        assert call(q=q) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(w=2, h=1, n=8192) == api.E_INVALID and b"ctx is NULL" in err()
    for pt, comp in ((0, 1), (2, 2), (1, 4)):
        assert call(pt=pt, pitch=8*4*comp + comp) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(src=None) == api.E_INVALID and b"src is NULL" in err()
    for w, h in ((1, 4), (0, 4), (8, 0), (32769, 4), (8, 32769)):
        assert call(w=w, h=h, pitch=1 << 30) == api.E_INVALID and b"width is 2 to" in err(), (w, h)
    for pt in (-1, 3):
        assert call(pt=pt) == api.E_INVALID and b"src_pixel_type" in err()
    assert call(pitch=8*16 - 4) == api.E_INVALID and b"src_pitch_bytes" in err() and b"a row" in err()
    assert call(pitch=8*16 + 2) == api.E_INVALID and b"src_pitch_bytes" in err() and b"aligned to a component" in err()
    assert call(src=pano.ctypes.data + 2) == api.E_INVALID and b"src not aligned" in err()
    for q in (0, 3, 8):
        assert call(q=q) == api.E_INVALID and b"supersample" in err()
    assert call(faces=None) == api.E_INVALID and b"faces is NULL" in err()
    for n in (0, 8193):
        assert call(n=n) == api.E_INVALID and b"face_size" in err()
    assert call(faces=ok["faces"][:3] + [None] + ok["faces"][4:]) == api.E_INVALID and b"faces[3] is NULL" in err()
    assert call(faces=ok["faces"][:5] + [ok["faces"][5] + 4]) == api.E_INVALID and b"faces[5] not aligned" in err()
    assert call(faces=[pano.ctypes.data] + ok["faces"][1:]) == api.E_INVALID and b"faces[0] equals src" in err()
    assert not pano.any() and not any(a.any() for a in faces)


def test_prefilter_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: _err(hip_lib)                            # noqa: E731
    N, L, K = 4, 3, 2
    src = [[np.zeros((max(1, N >> l), max(1, N >> l), 4), np.float32) for l in range(L)] for _ in range(6)]
    dst = [[np.full((max(1, N >> k), max(1, N >> k), 4), 7.0, np.float32) for k in range(K)] for _ in range(6)]
    table = envmap_ref.ggx_sample_table(0.5, 64, N, L)
    ok = dict(src=[a.ctypes.data for f in src for a in f], dst=[a.ctypes.data for f in dst for a in f], n=N, L=L, K=K,
              tables=[None, table], counts=[0, 64])

    def call(**kw):
        a = dict(ok, **kw)
        s = (ctypes.c_void_p*len(a["src"]))(*a["src"]) if a["src"] is not None else None
        d = (ctypes.c_void_p*len(a["dst"]))(*a["dst"]) if a["dst"] is not None else None
        keep = [None if t is None else np.ascontiguousarray(t, np.float32) for t in a["tables"]] if a["tables"] is not None else None
        t = (ctypes.c_void_p*len(keep))(*[None if x is None else x.ctypes.data for x in keep]) if keep is not None else None
        c = (ctypes.c_uint32*len(a["counts"]))(*a["counts"]) if a["counts"] is not None else None
        return hip_lib.cfhip_cube_prefilter_device(None, s, a["n"], a["L"], d, a["K"], t, c, None)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(tables=[table, table], counts=[64, 64]) == api.E_INVALID and b"ctx is NULL" in err()
    big = envmap_ref.ggx_sample_table(1.0, 4096, N, L)
    assert call(tables=[None, big], counts=[0, 4096]) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(src=None) == api.E_INVALID and b"src_levels is NULL" in err()
    assert call(dst=None) == api.E_INVALID and b"dst_levels is NULL" in err()
    assert call(tables=None) == api.E_INVALID and b"tables is NULL" in err()
    assert call(counts=None) == api.E_INVALID and b"table_samples is NULL" in err()
    for n in (0, 8193):
        assert call(n=n) == api.E_INVALID and b"face_size" in err()
    for levels in (0, 4):
        assert call(L=levels) == api.E_INVALID and b"source_levels" in err()
        assert call(K=levels) == api.E_INVALID and b"dst_count" in err()
    assert call(src=ok["src"][:4] + [None] + ok["src"][5:]) == api.E_INVALID and b"src_levels[1][1] is NULL" in err()
    assert call(src=[ok["src"][0] + 8] + ok["src"][1:]) == api.E_INVALID and b"src_levels[0][0] not aligned" in err()
    assert call(dst=ok["dst"][:11] + [None]) == api.E_INVALID and b"dst_levels[5][1] is NULL" in err()
    assert call(dst=ok["dst"][:2] + [ok["dst"][2] + 4] + ok["dst"][3:]) == api.E_INVALID and b"dst_levels[1][0] not aligned" in err()
    assert call(dst=ok["dst"][:3] + [ok["src"][7]] + ok["dst"][4:]) == api.E_INVALID \
        and b"dst_levels[1][1] equals src_levels[2][1]" in err()
    for count in (32, 100, 4160, 8192):
        assert call(counts=[0, count]) == api.E_INVALID and b"table_samples[1]" in err(), count
    assert call(tables=[None, None]) == api.E_INVALID and b"tables[1] is NULL" in err()
    # a copy needs its source level
    assert call(L=1, src=[f[0].ctypes.data for f in src], tables=[table, None], counts=[64, 0]) == api.E_INVALID \
        and b"a copy" in err()
    for field, value in ((0, np.nan), (1, np.inf), (2, -0.5), (2, np.nan), (3, -1.0), (3, 15.0), (3, np.nan)):
        bad = table.copy()
        bad[5, field] = value
        assert call(tables=[None, bad]) == api.E_INVALID and b"tables[1][5]" in err(), (field, value)
    assert all((a == 7.0).all() for f in dst for a in f) and not any(a.any() for f in src for a in f)


def test_sh9_argument_errors(hip_lib):
    from cuttlefish_amd import api
    err = lambda: _err(hip_lib)                            # noqa: E731
    faces = [np.zeros((2, 2, 4), np.float32) for _ in range(6)]
    res = np.zeros(37, np.float64)
    ok = dict(faces=[a.ctypes.data for a in faces], n=2, res=res.ctypes.data)

    def call(**kw):
        a = dict(ok, **kw)
        arr = (ctypes.c_void_p*6)(*a["faces"]) if a["faces"] is not None else None
        return hip_lib.cfhip_cube_sh9_device(None, arr, a["n"], a["res"], None)
    assert call() == api.E_INVALID and b"ctx is NULL" in err()
    assert call(n=8192) == api.E_INVALID and b"ctx is NULL" in err()
    assert call(faces=None) == api.E_INVALID and b"faces is NULL" in err()
    for n in (0, 8193):
        assert call(n=n) == api.E_INVALID and b"face_size" in err()
    assert call(faces=[None] + ok["faces"][1:]) == api.E_INVALID and b"faces[0] is NULL" in err()
    assert call(faces=ok["faces"][:2] + [ok["faces"][2] + 8] + ok["faces"][3:]) == api.E_INVALID and b"faces[2] not aligned" in err()
    assert call(res=None) == api.E_INVALID and b"result_device is NULL" in err()
    assert call(res=res.ctypes.data + 4) == api.E_INVALID and b"result_device not aligned" in err()
    assert not res.any()


@pytest.mark.parametrize("roughness", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("samples", [64, 256])
def test_the_c_table_helper_is_the_numpy_one_within_one_unit_in_the_last_place(hip_lib, roughness, samples):
    """the two call different cos, sin and log2: every field within one float32 unit in the last place"""
    from cuttlefish_amd import api
    for n, levels in ((256, 9), (16, 5), (5, 1)):
        got = api.ggx_sample_table(roughness, samples, n, levels)
        want = envmap_ref.ggx_sample_table(roughness, samples, n, levels)
        assert got.shape == want.shape == (samples, 4) and got.dtype == want.dtype == np.float32
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        assert (got[:, 2] == want[:, 2]).all()             # lz has no library call in it
        assert ((got[:, 2] == 0) == (want[:, 2] == 0)).all() and (got[want[:, 2] == 0, 3] == 0).all()


def test_the_c_table_helper_refuses_what_has_no_table(hip_lib):
    from cuttlefish_amd import api
    out = np.full((64, 4), 7.0, np.float32)
    p = out.ctypes.data_as(ctypes.POINTER(api.GgxSample))
    for r, s, n, levels in ((0.0, 64, 16, 5), (-1.0, 64, 16, 5), (1.5, 64, 16, 5), (float("nan"), 64, 16, 5), (0.5, 0, 16, 5),
                            (0.5, 32, 16, 5), (0.5, 96 + 1, 16, 5), (0.5, 8192, 16, 5), (0.5, 64, 0, 1), (0.5, 64, 8193, 1),
                            (0.5, 64, 16, 0), (0.5, 64, 16, 6)):
        assert hip_lib.cfhip_ggx_sample_table(r, s, n, levels, p) == api.E_INVALID, (r, s, n, levels)
    assert hip_lib.cfhip_ggx_sample_table(0.5, 64, 16, 5, None) == api.E_INVALID
    assert (out == 7.0).all()
    assert hip_lib.cfhip_ggx_sample_table(0.5, 64, 16, 5, p) == 0 and not (out == 7.0).any()
    for bad in (dict(roughness=0.0), dict(roughness=2.0), dict(samples=100), dict(samples=True), dict(samples=64.0),
                dict(face_size=0), dict(source_levels=9)):
        with pytest.raises(ValueError):
            api.ggx_sample_table(**dict(dict(roughness=0.5, samples=64, face_size=16, source_levels=5), **bad))


def test_python_surface():
    from cuttlefish_amd import ColorSpace, CubeFace, Dimension, Texture, api
    C = api.Context
    for f in (C.equirect_to_cube_device, C.equirect_to_cube, C.cube_prefilter_device, C.cube_prefilter, C.cube_sh9_device,
              C.cube_sh9, api.ggx_sample_table, api.sh9_irradiance, Texture.from_panorama, Texture.prefilter_environment,
              Texture.irradiance_sh9):
        assert callable(f)

    def params(f, skip=1):
        return [(n, p.default) for n, p in list(inspect.signature(f).parameters.items())[skip:]]
    E = inspect.Parameter.empty
    assert params(C.equirect_to_cube_device) == [("src", E), ("pixel_type", E), ("width", E), ("height", E), ("row_pitch_bytes", E),
                                                 ("faces", E), ("face_size", E), ("supersample", 2), ("stream", 0)]
    assert params(C.equirect_to_cube) == [("image", E), ("face_size", E), ("supersample", 2)]
    assert params(C.cube_prefilter_device) == [("src_levels", E), ("face_size", E), ("dst_levels", E), ("tables", E), ("stream", 0)]
    assert params(C.cube_prefilter) == [("faces", E), ("roughness", E), ("samples", 256)]
    assert params(C.cube_sh9_device) == [("faces", E), ("face_size", E), ("result", E), ("stream", 0)]
    assert params(C.cube_sh9) == [("faces", E)]
    assert params(api.ggx_sample_table, 0) == [("roughness", E), ("samples", E), ("face_size", E), ("source_levels", E)]
    assert params(Texture.from_panorama, 0)[:4] == [("image", E), ("face_size", E), ("supersample", 2),
                                                    ("color_space", ColorSpace.Linear)]
    assert params(Texture.prefilter_environment) == [("mip_levels", None), ("samples", 256), ("roughness", None)]
    assert params(Texture.irradiance_sh9) == []
    assert api.cube_level_count(1) == 1 and api.cube_level_count(16) == 5 and api.cube_level_count(17) == 5
    # what is no complete cube is refused before any device work
    flat = Texture(8, 8)
    assert flat.set_image(np.zeros((8, 8, 4), np.float32))
    cube = Texture(Dimension.Cube, 8, 8)
    assert cube.set_image(np.zeros((8, 8, 4), np.float32), CubeFace.PosX)
    array = Texture(Dimension.Cube, 8, 8, 2)
    for t in (Texture(), flat, cube, array):
        assert t.prefilter_environment() is False and t.irradiance_sh9() is None
    assert Texture.from_panorama(np.zeros((4, 8), np.float32), 4) is None
    # the host helper: a constant environment is lit by pi times itself from every side
    coeffs = envmap_ref.sh9(np.full((6, 4, 4, 4), 0.5, np.float32))[:36].reshape(9, 4)
    d = np.array([[1.0, 0, 0], [0, -1.0, 0], [0.6, 0, 0.8]])
    assert np.abs(api.sh9_irradiance(coeffs, d) - 0.5*np.pi).max() < 1e-12
    assert np.abs(api.sh9_irradiance(coeffs, d) - envmap_ref.sh9_irradiance(coeffs, d)).max() < 1e-15
    with pytest.raises(ValueError):
        api.sh9_irradiance(np.zeros((8, 4)), d)
