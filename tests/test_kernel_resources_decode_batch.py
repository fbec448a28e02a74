"""The batched decode kernels in the built code object: no scratch, no spilled vector register, no AGPR; the
instantiations that exist; and the census of the per-surface decode kernels is untouched."""
import pytest


def test_batched_decode_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    block = {k: v for k, v in meta.items() if "cfhip_decode_batch_kernel" in k}
    astc = {k: v for k, v in meta.items() if "cfhip_decode_batch_astc_kernel" in k}
    # 19 (format, type) pairs x {native, RGBA32F} + BC4 / BC5 UNorm expanded to RGBA8; ASTC: 2 profiles x 2 outputs
    assert len(block) == 19*2 + 2, sorted(block)
    assert len(astc) == 4, sorted(astc)
    for k, v in {**block, **astc}.items():
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
        assert not any(s in k for s in ("cfhip_decode_block_kernel", "cfhip_decode_astc_kernel", "cfhip_decode_sse_",
                                        "cfhip_compare_", "_encode_kernel")), k
    for stem in ("cfhip_decode_batch_kernel", "cfhip_decode_batch_astc_kernel"):
        assert stem in build.BLOCK_KERNELS
    assert len([k for k in meta if "cfhip_decode_block_kernel" in k]) == 19
    assert len([k for k in meta if "cfhip_decode_astc_kernel" in k]) == 2
