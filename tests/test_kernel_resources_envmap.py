"""The environment-map kernels in the built code object: no scratch, no spilled vector register, no AGPR, exactly the LDS
that DESIGN.md section 4.23 states -- the panorama pass's table of 8-bit components, the prefilter's staged sample records
and chain pointers, the final sum's one double -- and registers for four waves per SIMD where the work is heavy."""
import pytest


def test_envmap_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # equirect: the 256 float values of an 8-bit component; prefilter: 1024 records of 16 bytes and 6 x 14 pointers;
    # final: the summed solid angle
    lds = {"cfhip_equirect_to_cube_kernel": 256*4, "cfhip_cube_prefilter_kernel": 1024*16 + 6*14*8, "cfhip_cube_copy_kernel": 0,
           "cfhip_cube_sh9_rows_kernel": 0, "cfhip_cube_sh9_final_kernel": 8}
    for name, want in lds.items():
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == 1, (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            assert v["lds"] == want, (k, v)
            if name in ("cfhip_cube_prefilter_kernel", "cfhip_cube_sh9_rows_kernel"):
                assert v["vgpr"] <= 128, (k, v)                # four waves per SIMD
    build.check_no_vector_spills()
