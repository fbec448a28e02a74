"""The batched compare kernels in the built code object: no scratch, no spilled vector register, no AGPR; the
instantiations that exist; the same LDS as the per-surface kernels whose work they share; and the census of the
per-surface compare kernels is untouched."""
import pytest


def test_batched_compare_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")

    def named(stem):
        return {k: v for k, v in meta.items() if stem in k}
    block, astc = named("cfhip_compare_batch_block_kernel"), named("cfhip_compare_batch_astc_kernel")
    ssim, final = named("cfhip_compare_batch_ssim_kernel"), named("cfhip_compare_batch_final_kernel")
    # the 19 lane-per-block (format, type) pairs; ASTC LDR and HDR; one SSIM and one final kernel
    assert (len(block), len(astc), len(ssim), len(final)) == (19, 2, 1, 1), sorted(meta)
    for k, v in {**block, **astc, **ssim, **final}.items():
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
    for stem in ("cfhip_compare_batch_block_kernel", "cfhip_compare_batch_astc_kernel",
                 "cfhip_compare_batch_ssim_kernel", "cfhip_compare_batch_final_kernel"):
        assert stem in build.BLOCK_KERNELS
    # the per-surface kernels are thin wrappers around the same __device__ functions: same census, same LDS
    single = {stem: named(stem) for stem in ("cfhip_compare_block_kernel", "cfhip_compare_astc_kernel",
                                             "cfhip_compare_ssim_kernel", "cfhip_compare_final_kernel")}
    assert [len(v) for v in single.values()] == [19, 2, 1, 1]
    for one, many in zip(single.values(), (block, astc, ssim, final)):
        assert sorted(v["lds"] for v in one.values()) == sorted(v["lds"] for v in many.values())
