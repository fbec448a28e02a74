"""The rate-distortion kernel in the built code object: one instantiation per row of the table, no scratch, no
spilled vector register, no AGPR, and the ring of the last L final blocks as its only LDS."""
import pytest

import rdo_ref


def test_rdo_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    rdo = {k: v for k, v in meta.items() if "cfhip_rdo_kernel" in k}
    assert len(rdo) == len(rdo_ref.TABLE) == 7, sorted(meta)
    assert "cfhip_rdo_kernel" in build.BLOCK_KERNELS
    for k, v in rdo.items():
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
        # four wavefronts a workgroup, L slots of 16 bytes each: at most 256 bytes per wavefront
        assert v["lds"] == 4*rdo_ref.L*16 and rdo_ref.L*16 <= 256, (k, v)
        assert v["vgpr"] <= 128, (k, v)          # four waves per SIMD at least
    build.check_no_vector_spills()
