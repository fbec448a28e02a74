"""The C-ABI library loads and exports every symbol include/cuttlefish_hip.h declares.
No compute calls here (this file runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cfhip_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_expected_entry_points():
    from cuttlefish_amd import api
    assert _declared_symbols() == sorted(api.EXPORTS)


def test_library_exports_every_declared_symbol(hip_lib):
    for name in _declared_symbols():
        assert hasattr(hip_lib, name), name


def test_abi_version_and_query(hip_lib):
    from cuttlefish_amd import api
    assert hip_lib.cfhip_abi_version() == 1
    # Texture::blockSize (Texture.cpp:693-773)
    assert api.query(api.Format.BC7, api.Type.UNorm) == (4, 4, 16)
    assert api.query(api.Format.BC1_RGB, api.Type.UNorm) == (4, 4, 8)
    assert api.query(api.Format.BC4, api.Type.SNorm) == (4, 4, 8)
    assert api.query(api.Format.BC6H, api.Type.UFloat) == (4, 4, 16)
    # createConverter returns nullptr for these (Converter.cpp:339-412)
    for fmt, typ in [(api.Format.BC7, api.Type.SNorm), (api.Format.BC1_RGB, api.Type.Float),
                     (api.Format.BC6H, api.Type.UNorm), (api.Format.BC4, api.Type.UFloat)]:
        with pytest.raises(api.CfhipError):
            api.query(fmt, typ)


def test_shard_rows_partition_is_exact(hip_lib):
    from cuttlefish_amd import api
    for rows in (1, 7, 1024, 1025):
        for world in (1, 2, 3, 8):
            spans = [api.shard_rows(rows, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == rows
            for a, b in zip(spans, spans[1:]):
                assert a[1] == b[0]
    with pytest.raises(api.CfhipError):
        api.shard_rows(8, 2, 2)


def test_no_device_fails_loudly(hip_lib):
    """No CPU fallback: without a HIP device context creation must fail."""
    from cuttlefish_amd import api
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(api.CfhipError):
        api.Context(0)


def test_texture_convert_rejects_illegal_combinations(hip_lib):
    """Texture::convert returns false before touching the device for illegal input
    (Texture.cpp:1539-1543)."""
    import numpy as np
    from cuttlefish_amd import ColorSpace, Format, Texture, Type
    t = Texture(16, 16)
    assert not t.convert(Format.BC7, Type.UNorm)          # images incomplete
    assert t.set_image(np.zeros((16, 16, 4), np.float32))
    assert not t.convert(Format.BC7, Type.SNorm)          # illegal type
    assert not t.set_image(np.zeros((8, 16, 4), np.float32))
    s = Texture(16, 16, color_space=ColorSpace.sRGB)
    assert s.set_image(np.zeros((16, 16, 4), np.float32))
    assert not s.convert(Format.BC4, Type.UNorm)          # no native sRGB (Texture.cpp:421-465)


def test_query_accepts_exactly_the_pairs_the_reference_convert_tests_list(hip_lib):
    """lib/test/TextureTest.cpp:869-985 instantiates TextureConvertTest / TextureConvertSpecialTest
    with every (format, type) pair Texture::convert must accept (fixture
    tests/golden/convert_expectations.json, extracted by tests/golden/make_convert_expectations.py);
    createConverter answers nullptr for every other pair.  cfhip_query is the backend's statement
    of the same matrix (no GPU needed).  PVRTC is the one family this backend does not have."""
    import json
    from cuttlefish_amd import api
    listed = set(json.load(open(os.path.join(ROOT, "tests", "golden", "convert_expectations.json"))))
    listed = {p for p in listed if not p.startswith("PVRTC")}
    # ASTC_6x6 is missing from the reference's list (TextureTest.cpp:941-954) although legal
    listed |= {"ASTC_6x6/UNorm", "ASTC_6x6/UFloat"}
    accepted = set()
    for fmt in api.Format:
        for typ in api.Type:
            try:
                api.query(fmt, typ)
                accepted.add("%s/%s" % (fmt.name, typ.name))
            except api.CfhipError:
                pass
    assert accepted == listed, (sorted(accepted - listed), sorted(listed - accepted))


def test_mip_and_resize_calls_without_a_context_are_invalid(hip_lib):
    """cfhip_generate_mips_device, its array and 3-D forms and cfhip_resize_device check the context before any
    argument: without one the answer is CFHIP_E_INVALID "ctx is NULL", also where an argument is NULL or empty as
    well (with a context those draw the call's own "... NULL or empty argument")."""
    from cuttlefish_amd import api
    L = hip_lib
    buf = (ctypes.c_uint8 * 256)()
    src = ctypes.cast(buf, ctypes.c_void_p)
    one = (ctypes.c_void_p * 1)(src)
    rgba8, linear, box = int(api.PixelType.RGBA8), int(api.ColorSpace.Linear), 0
    for s, w, tab in [(src, 4, one), (None, 4, one), (src, 0, one), (src, 4, None)]:
        calls = {
            "generate_mips": lambda: L.cfhip_generate_mips_device(None, s, rgba8, w, 4, 16, linear, box, tab, 2, None),
            "generate_mips_array": lambda: L.cfhip_generate_mips_array_device(
                None, one if s else None, 1, rgba8, w, 4, 16, linear, box, tab, 2, None),
            "generate_mips3d": lambda: L.cfhip_generate_mips3d_device(
                None, s, rgba8, w, 4, 2, 16, 64, linear, box, tab, 2, None),
            "resize": lambda: L.cfhip_resize_device(None, s, rgba8, w, 4, 16, linear, box, src if tab else None, 2, 2, None),
        }
        for name, call in calls.items():
            assert call() == api.E_INVALID, (name, s, w, tab)
            assert L.cfhip_last_error(None) == b"ctx is NULL", (name, s, w, tab)


def test_header_compiles_as_plain_c99(tmp_path):
    """integration/check_header.c: a C translation unit including include/cuttlefish_hip.h,
    -std=c99 -pedantic-errors (the boundary is a C ABI, not a C++ one)."""
    import subprocess
    src = os.path.join(ROOT, "integration", "check_header.c")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-c",
                           "-I" + os.path.join(ROOT, "include"), src, "-o", str(tmp_path / "h.o")])


def test_graft_entry_module_imports():
    """the driver imports __graft_entry__ and calls build(): a syntax error there hides every
    later source change behind a stale library"""
    import importlib
    import __graft_entry__
    importlib.reload(__graft_entry__)
    assert callable(__graft_entry__.build) and callable(__graft_entry__.smoke)
