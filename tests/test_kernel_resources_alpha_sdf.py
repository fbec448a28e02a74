"""The distance field's kernels in the built code object: no scratch, no spilled vector register, no AGPR, exactly the
LDS that DESIGN.md section 4.22 states -- the classify pass's table of 8-bit alphas and its count, the column pass's
staged rows and its count -- and few enough registers for full occupancy."""
import pytest


def test_alpha_sdf_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # row: with and without a wrapped x axis; column: storing the field (scale 1) or e
    want = {"cfhip_alpha_sdf_classify_kernel": 1, "cfhip_alpha_sdf_row_kernel": 2, "cfhip_alpha_sdf_column_kernel": 2,
            "cfhip_alpha_sdf_resolve_kernel": 1}
    # classify: the 256 float values of an 8-bit alpha and the workgroup's count; column: 64 + 2 * 126 rows of 64 bytes
    # and the workgroup's count
    lds = {"cfhip_alpha_sdf_classify_kernel": 256*4 + 4, "cfhip_alpha_sdf_row_kernel": 0,
           "cfhip_alpha_sdf_column_kernel": (64 + 2*126)*64 + 4, "cfhip_alpha_sdf_resolve_kernel": 0}
    for name, count in want.items():
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == count, (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            assert v["lds"] == lds[name] and v["vgpr"] <= 64, (k, v)
    build.check_no_vector_spills()
