"""The kernels of the height-map ambient occlusion in the built code object: no scratch, no spilled vector register, no
AGPR, at most 128 VGPRs, and exactly the LDS that DESIGN.md section 4.25 and csrc/height_ao.h state -- per halo class
the tile (64 x 16 texels up to R = 16, 64 x 64 above) with the class's halo on every side, one float a texel, and the
workgroup's two record words; the plane kernel holds the table of the 256 decoded 8-bit values."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_height_ao_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    scan = {halo: (64 + 2*halo)*((16 if halo == 16 else 64) + 2*halo)*4 + 8 for halo in (16, 32, 64)}
    assert scan == {16: 18440, 32: 65544, 64: 147464}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.25"):]
    shared = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "height_ao.h")).read()
    for text in (section, shared):
        for lds in scan.values():
            assert re.search(r"%d[ ,]?%03d\b" % divmod(lds, 1000), text), lds
    assert "CFHAO_HALO_CLASSES[3] = {16, 32, 64};" in shared
    assert "(CFHAO_TILE_W + 2u*halo)*(cfhao_tile_rows(halo) + 2u*halo)*4u + 8u" in shared
    assert "return halo <= CFHAO_HALO_CLASSES[0] ? CFHAO_TILE_H : CFHAO_TILE_H_WIDE;" in shared
    assert int(re.search(r"CFHAO_TILE_W = (\d+);", shared).group(1)) == 64
    assert int(re.search(r"CFHAO_TILE_H = (\d+);", shared).group(1)) == 16
    assert int(re.search(r"CFHAO_TILE_H_WIDE = (\d+);", shared).group(1)) == 64
    want = {"cfhip_height_ao_plane_kernel": [256*4], "cfhip_height_ao_scan_kernel": sorted(scan.values())}
    for name, lds in want.items():
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert sorted(v["lds"] for v in found.values()) == lds, (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            assert v["vgpr"] <= 128, (k, v)
    build.check_no_vector_spills()
