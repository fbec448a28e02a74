"""The kernels of specular anti-aliasing in the built code object: no scratch, no spilled vector register, no AGPR, and
exactly the LDS that DESIGN.md section 4.24 states -- a tile's moments on five levels, the workgroup's share of five
records and, where a surface is 8-bit, the table of its 256 decoded values."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spec_aa_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # int64 sums, four planes: at most 31^2 + 15^2 + 7^2 + 3^2 + 1 texels of a tile's five levels; 16 words of records
    base = (31*31 + 15*15 + 7*7 + 3*3 + 1)*4*8 + 16*4
    table = 256*4
    assert base == 39904
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.24"):]
    assert re.search(r"39[ ,]?904", section) and re.search(r"40[ ,]?928", section)
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "spec_aa.h")).read()
    assert "CFSA_LDS_ENTRIES = 31u*31u + 15u*15u + 7u*7u + 3u*3u + 1u;" in shared
    # texel: three pixel types of the normals x (no roughness map, or one of three pixel types); 8-bit normals (4) and
    # 8-bit roughness under other normals (2) hold the table
    want = {"cfhip_spec_aa_texel_kernel": sorted([base]*6 + [base + table]*6), "cfhip_spec_aa_moment_kernel": [base]}
    for name, lds in want.items():
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert sorted(v["lds"] for v in found.values()) == lds, (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            assert v["vgpr"] <= 128, (k, v)            # two workgroups of 256 per SIMD-quad at the least
    build.check_no_vector_spills()
