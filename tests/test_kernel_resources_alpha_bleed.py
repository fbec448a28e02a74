"""Alpha bleeding's kernels in the built code object: no scratch, no spilled vector register, no AGPR, no LDS beyond the
seed pass's table of 8-bit alphas and the workgroup sums of the two counting passes, and few enough registers for full
occupancy."""
import pytest


def test_alpha_bleed_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # step and fill: with and without a wrapped axis
    want = {"cfhip_alpha_bleed_seed_kernel": 1, "cfhip_alpha_bleed_step_kernel": 2, "cfhip_alpha_bleed_fill_kernel": 2}
    # seed: the 256 float values of an 8-bit alpha and the workgroup's count; fill: its count and its maximum
    lds = {"cfhip_alpha_bleed_seed_kernel": 256*4 + 4, "cfhip_alpha_bleed_step_kernel": 0, "cfhip_alpha_bleed_fill_kernel": 8}
    for name, count in want.items():
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == count, (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            assert v["lds"] == lds[name] and v["vgpr"] <= 64, (k, v)
    build.check_no_vector_spills()
