"""The lookup-table and irradiance kernels in the built code object: no scratch, no spilled vector register, no AGPR, and
exactly the LDS that DESIGN.md section 4.27 states -- the lookup table's staged Hammersley records, nothing for the
irradiance cube, whose coefficients arrive by scalar loads."""
import pytest


def test_envlobe_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # lookup table: 1024 records of 16 bytes, with and without the sheen column; irradiance: none
    for name, count, lds in (("cfhip_brdf_lut_kernel", 2, 1024*16), ("cfhip_cube_irradiance_kernel", 1, 0)):
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == count, (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            assert v["lds"] == lds, (k, v)
            assert v["vgpr"] <= 128, (k, v)                    # four waves per SIMD, pow included
    build.check_no_vector_spills()
