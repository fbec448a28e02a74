"""The 2-D rate-distortion kernel in the built code object: one instantiation per row of the table, no scratch, no
spilled vector register, no AGPR, and the ring plus one row of final blocks per wavefront as its only LDS."""
import pytest

import rdo_ref


def test_rdo2d_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    rdo = {k: v for k, v in meta.items() if "cfhip_rdo2d_kernel" in k}
    assert len(rdo) == len(rdo_ref.TABLE) == 7, sorted(meta)
    assert "cfhip_rdo2d_kernel" in build.BLOCK_KERNELS
    for k, v in rdo.items():
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
        # four wavefronts a workgroup, each with L ring slots and SEG blocks of the row above, 16 bytes each
        assert v["lds"] == 4*(rdo_ref.L + rdo_ref.SEG)*16 <= 8192, (k, v)
    build.check_no_vector_spills()
