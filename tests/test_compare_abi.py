"""The quality-metric entry points of the C-ABI without a GPU: declared and exported, the ctypes struct laid out as
the header's, the argument checks that answer before any device work, and the kernels' resources."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cuttlefish_hip.h")
NAMES = ("cfhip_compare", "cfhip_compare_device")


def test_header_declares_and_library_exports_compare(hip_lib):
    from cuttlefish_amd import api
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(cfhip_[a-z_0-9]+)\s*\(", text))
    for n in NAMES:
        assert n in declared and n in api.EXPORTS and hasattr(hip_lib, n), n
    assert re.search(r"#define\s+CFHIP_COMPARE_SSIM\s+1u", text)
    assert api.COMPARE_SSIM == 1


def test_struct_layout_matches_header(tmp_path):
    from cuttlefish_amd import api
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in api.CompareResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu\\n", sizeof(cfhip_compare_result));\n%s  return 0;\n}\n' %
                   (HEADER, "".join('  printf("%%zu\\n", offsetof(cfhip_compare_result, %s));\n' % f
                                    for f in fields)))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(api.CompareResult) == 152
    assert got[1:] == [getattr(api.CompareResult, f).offset for f in fields]


def _call(L, ctx, fmt, typ, w=8, h=8, ref_pix=0):
    from cuttlefish_amd import api
    blocks = np.zeros(4096, np.uint8)
    ref = np.zeros((h, w, 4), np.uint8)
    res = api.CompareResult()
    return L.cfhip_compare(ctx, fmt, typ, blocks.ctypes.data, blocks.nbytes, w, h, ref.ctypes.data, ref_pix, w * 4,
                           None, 0, ctypes.byref(res), None, 0)


def test_null_context_is_invalid(hip_lib):
    from cuttlefish_amd import api
    assert _call(hip_lib, None, 29, 0) == api.E_INVALID
    res = api.CompareResult()
    assert hip_lib.cfhip_compare_device(None, 29, 0, None, 8, 8, None, 0, 32, None, 0, ctypes.byref(res), None, 0,
                                        None) == api.E_INVALID


@pytest.mark.parametrize("fmt,typ", [(14, 0), (10, 0), (22, 4), (29, 1), (36, 4), (35, 0), (43, 1), (41, 4)])
def test_standard_formats_and_rejected_pairs_have_no_layout(hip_lib, fmt, typ):
    from cuttlefish_amd import api
    # cfhip_compare answers E_UNSUPPORTED for exactly the pairs without a decoded layout (its checks start from
    # decode_check's); a context needs a device, so here the table is asked directly and through the Python path
    # Context.compare takes first (tests/test_gpu_compare.py asks cfhip_compare itself)
    assert hip_lib.cfhip_decoded_layout(fmt, typ, None, None) == api.E_UNSUPPORTED
    with pytest.raises(api.CfhipError) as e:
        api.decoded_layout(fmt, typ)
    assert e.value.code == api.E_UNSUPPORTED


def test_compare_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    for name in ("cfhip_compare_block_kernel", "cfhip_compare_astc_kernel", "cfhip_compare_ssim_kernel",
                 "cfhip_compare_final_kernel"):
        assert name in build.BLOCK_KERNELS
        ks = {k: v for k, v in meta.items() if name in k}
        assert ks, name
        for k, v in ks.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
    assert len([k for k in meta if "cfhip_compare_block_kernel" in k]) == 19     # one per 4x4 (format, type) pair
    assert len([k for k in meta if "cfhip_compare_astc_kernel" in k]) == 2      # LDR and HDR profiles
