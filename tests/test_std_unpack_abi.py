"""The standard-format unpack and compare entry points of the C-ABI without a GPU: declared and exported, the
legality table they follow, the answers that need no device, and the kernels' resources."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_oracle_stdpack import ALL_PAIRS, LEGAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cuttlefish_hip.h")
NAMES = ("cfhip_std_unpack", "cfhip_std_unpack_device", "cfhip_std_compare", "cfhip_std_compare_device")


def test_header_declares_and_library_exports_the_std_entry_points(hip_lib):
    from cuttlefish_amd import api
    from test_abi import _declared_symbols
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(cfhip_[a-z_0-9]+)\s*\(", text))
    for n in NAMES:
        assert n in declared and n in api.EXPORTS and hasattr(hip_lib, n), n
    assert _declared_symbols() == sorted(api.EXPORTS)
    assert re.search(r"CFHIP_LAYOUT_RGBA32F\s*=\s*10\b", text)
    assert api.Layout.RGBA32F == 10 and api.LAYOUT_ARRAY[api.Layout.RGBA32F] == (4, np.float32)
    assert re.search(r"#define\s+CFHIP_ABI_VERSION\s+1\b", text) and hip_lib.cfhip_abi_version() == 1


def test_legality_is_cfhip_querys_for_formats_1_to_28(hip_lib):
    from cuttlefish_amd import api
    legal = []
    for f in range(0, 64):
        for t in range(6):
            bs = ctypes.c_int()
            rc = hip_lib.cfhip_query(f, t, None, None, ctypes.byref(bs))
            if 1 <= f <= 28:
                assert (rc == 0) == (t in LEGAL.get(f, {})), (f, t)
                if rc == 0:
                    assert bs.value == LEGAL[f][t]
                    legal.append((f, t))
                else:
                    assert rc == api.E_UNSUPPORTED
    assert legal == ALL_PAIRS and len(legal) == 66


def test_the_generic_entries_still_have_no_layout_for_standard_formats(hip_lib):
    from cuttlefish_amd import api
    for f, t in ALL_PAIRS:
        assert hip_lib.cfhip_decoded_layout(f, t, None, None) == api.E_UNSUPPORTED


def test_std_calls_without_a_context_are_invalid(hip_lib):
    from cuttlefish_amd import api
    px = np.zeros(64, np.uint8)
    out = np.zeros((4, 4, 4), np.float32)
    res = api.CompareResult()
    assert hip_lib.cfhip_std_unpack(None, 14, 0, px.ctypes.data, px.nbytes, 4, 4, out.ctypes.data,
                                    out.nbytes) == api.E_INVALID
    assert hip_lib.cfhip_std_unpack_device(None, 14, 0, None, 4, 4, None, 64, None) == api.E_INVALID
    assert hip_lib.cfhip_std_compare(None, 14, 0, px.ctypes.data, px.nbytes, 4, 4, px.ctypes.data, 0, 16, None, 0,
                                     ctypes.byref(res)) == api.E_INVALID
    assert hip_lib.cfhip_std_compare_device(None, 14, 0, None, 4, 4, None, 0, 16, None, 0, None,
                                            None) == api.E_INVALID
    assert b"ctx is NULL" in hip_lib.cfhip_last_error(None)


def test_comparison_peak_of_the_standard_types():
    from cuttlefish_amd import api
    res = api.CompareResult()
    res.channels = 0b0111
    res.texels = 4
    for c, v in enumerate((3.0, 9.0, 5.0, 100.0)):
        res.ref_max[c] = v
    assert api.Comparison(res, api.Layout.RGBA32F, typ=api.Type.UNorm).peak() == 1.0
    assert api.Comparison(res, api.Layout.RGBA32F, typ=api.Type.SNorm).peak() == 2.0
    for t in (api.Type.UInt, api.Type.Int, api.Type.Float, api.Type.UFloat):
        assert api.Comparison(res, api.Layout.RGBA32F, typ=t).peak() == 9.0          # alpha is not compared
        assert api.Comparison(res, api.Layout.RGBA32F, typ=t).peak([0, 2]) == 5.0
    assert api.Comparison(res, api.Layout.RGBA8).peak() == 1.0                       # block layouts: unchanged
    assert api.Comparison(res, api.Layout.RG8_SNorm).peak() == 2.0
    assert api.Comparison(res, api.Layout.RGBA16F).peak() == 9.0


def test_std_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    for name in ("cfhip_std_unpack_kernel", "cfhip_std_compare_kernel"):
        assert name in build.BLOCK_KERNELS
        ks = {k: v for k, v in meta.items() if name in k}
        assert len(ks) == 8, (name, sorted(ks))                      # one per pixel size: 1 2 3 4 6 8 12 16 bytes
        for k, v in ks.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            assert v["lds"] <= 4096, (k, v)
    # the census the other suites pin is untouched
    assert len([k for k in meta if "cfhip_decode_block_kernel" in k]) == 19
    assert len([k for k in meta if "cfhip_compare_block_kernel" in k]) == 19
    assert len([k for k in meta if "cfhip_compare_astc_kernel" in k]) == 2
    stems = ("cfhip_decode_block_kernel", "cfhip_compare_block_kernel", "cfhip_compare_astc_kernel", "_encode_kernel",
             "cfhip_std_pack_kernel")
    for k in meta:
        if "cfhip_std_unpack" in k or "cfhip_std_compare" in k:
            assert not any(s in k for s in stems), k
