"""The decode entry points of the C-ABI without a GPU: declared, exported, the layout table of every
(format, type) pair, and the decode kernels' resources read from the built code objects."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_ENTRY_POINTS = ["cfhip_decoded_layout", "cfhip_decode", "cfhip_decode_device", "cfhip_decode_sse",
                       "cfhip_decode_sse_device"]


def _declared():
    text = open(os.path.join(ROOT, "include", "cuttlefish_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(cfhip_[a-z_0-9]+)\s*\(", text))


def test_header_declares_and_library_exports_the_decode_entry_points(hip_lib):
    from cuttlefish_amd import api
    declared = _declared()
    for name in DECODE_ENTRY_POINTS:
        assert name in declared, name
        assert name in api.EXPORTS, name
        assert hasattr(hip_lib, name), name


def _expected_layout(fmt, typ):
    from cuttlefish_amd.api import Format as F, Layout as L, Type as T
    sn = typ == T.SNorm
    if fmt == F.BC4:
        return (L.R8_SNorm if sn else L.R8), 1
    if fmt == F.BC5:
        return (L.RG8_SNorm if sn else L.RG8), 2
    if fmt == F.EAC_R11:
        return (L.R16_SNorm if sn else L.R16), 2
    if fmt == F.EAC_R11G11:
        return (L.RG16_SNorm if sn else L.RG16), 4
    if fmt == F.BC6H or (fmt >= F.ASTC_4x4 and typ == T.UFloat):
        return L.RGBA16F, 8
    return L.RGBA8, 4


def test_decoded_layout_table(hip_lib):
    from cuttlefish_amd import api
    accepted = 0
    for fmt in range(29, 57):
        for typ in range(6):
            lay, tb = ctypes.c_int(-7), ctypes.c_int(-7)
            rc = hip_lib.cfhip_decoded_layout(fmt, typ, ctypes.byref(lay), ctypes.byref(tb))
            if hip_lib.cfhip_query(fmt, typ, None, None, None) != 0:
                assert rc == api.E_UNSUPPORTED, (fmt, typ)
                continue
            accepted += 1
            assert rc == 0, (fmt, typ)
            assert (lay.value, tb.value) == _expected_layout(fmt, typ), (fmt, typ)
            assert api.decoded_layout(fmt, typ) == _expected_layout(fmt, typ)
    # BC1 x2, BC2, BC3, BC7, ETC x4: 1 type; BC4, BC5, EAC x2: 2; BC6H: 2; ASTC x14: 2
    assert accepted == 9 + 8 + 2 + 28
    for fmt in range(1, 29):                       # the standard formats decode nothing
        for typ in range(6):
            assert hip_lib.cfhip_decoded_layout(fmt, typ, None, None) == api.E_UNSUPPORTED, (fmt, typ)
    for fmt, typ in [(0, 0), (57, 0), (36, 1), (35, 0), (33, 4), (43, 1), (-1, 0)]:
        assert hip_lib.cfhip_decoded_layout(fmt, typ, None, None) == api.E_UNSUPPORTED, (fmt, typ)
    with pytest.raises(api.CfhipError):
        api.decoded_layout(api.Format.BC7, api.Type.SNorm)


def test_decode_calls_without_a_context_are_invalid(hip_lib):
    from cuttlefish_amd import api
    buf = (ctypes.c_uint8 * 64)()
    assert hip_lib.cfhip_decode(None, 36, 0, buf, 64, 4, 4, buf, 64, None) == api.E_INVALID
    assert hip_lib.cfhip_decode_sse(None, 36, 0, buf, 64, 4, 4, buf, 16, (ctypes.c_uint64 * 4)()) == api.E_INVALID
    assert hip_lib.cfhip_decode_device(None, 36, 0, buf, 4, 4, buf, 16, None, None) == api.E_INVALID
    assert hip_lib.cfhip_decode_sse_device(None, 36, 0, buf, 4, 4, buf, 16, buf, None) == api.E_INVALID


def test_psnr_from_sse():
    from cuttlefish_amd import api
    assert api.psnr_from_sse([0, 0, 0, 5], 16) == float("inf")
    # one unit of error per texel and channel: 20 log10(255)
    assert abs(api.psnr_from_sse([16, 16, 16, 0], 16) - 48.1308) < 1e-3
    assert abs(api.psnr_from_sse([16, 0, 0, 0], 16, channels=1) - 48.1308) < 1e-3


def test_decode_kernels_use_no_scratch_no_spill_no_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools not present")
    for stem in ("cfhip_decode_block_kernel", "cfhip_decode_astc_kernel", "cfhip_decode_sse_block_kernel",
                 "cfhip_decode_sse_astc_kernel"):
        ks = {k: v for k, v in meta.items() if stem in k}
        assert ks, stem
        bad = {k: v for k, v in ks.items() if v["scratch"] != 0 or v["vgpr_spill"] != 0 or v["agpr"] != 0}
        assert not bad, bad
        assert any(s in stem for s in build.BLOCK_KERNELS)
    # lane-per-block kernels: one instantiation per (format, type) pair of the 4x4 families
    assert len([k for k in meta if "cfhip_decode_block_kernel" in k]) == 19
    # and none of them is counted as an encoder (tests/test_kernel_resources.py matches the encode stems)
    encode = ("cfhip_bc7_encode_kernel", "cfhip_bc15_encode_kernel", "cfhip_bc6h_encode_kernel",
              "cfhip_etc_encode_kernel", "cfhip_astc_encode_kernel")
    assert not [k for k in meta if "decode" in k and any(e in k for e in encode)]
