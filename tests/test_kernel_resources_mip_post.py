"""The mip post-pass's kernels in the built code object: no scratch, no spilled vector register, no AGPR, no LDS beyond
the gather pass's table (the counts are summed with ballots in scalar registers), and few enough registers for full
occupancy."""
import pytest


def test_mip_post_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # apply: with and without the renormalisation
    want = {"cfhip_mip_post_gather_kernel": 1, "cfhip_mip_post_count_kernel": 1, "cfhip_mip_post_decide_kernel": 1,
            "cfhip_mip_post_apply_kernel": 2}
    for name, count in want.items():
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == count, (name, sorted(found))
        for k, v in found.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            # gather: the 256 float values of an 8-bit alpha; the others none
            assert v["lds"] == (256*4 if "gather" in name else 0) and v["vgpr"] <= 64, (k, v)
    build.check_no_vector_spills()
