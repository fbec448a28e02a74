"""The inflater's kernels in the built code object: no scratch, no spilled vector register, no AGPR, and the LDS each
one was designed around (tests/test_kernel_resources_deflate.py reads the encoder's the same way)."""
import pytest

KERNELS = ("cfhip_inflate_decode_kernel", "cfhip_inflate_resolve_kernel", "cfhip_inflate_pack_kernel",
           "cfhip_inflate_fold_kernel", "cfhip_inflate_final_kernel", "cfhip_zindex_kernel")


def test_inflate_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # decode: CfinfWork (csrc/inflate.h) -- the chunk's 4096 words padded by one per 64 (16640 bytes), three canonical
    # codes (2722 bytes with a 10-bit first-level table, 674 with an 8-bit one, 392 with a 7-bit one), 340 code lengths,
    # 64 cover entries, 88 bytes of the walk's state: seven wavefronts per CU, so LDS bounds the occupancy before the
    # registers do (256 VGPRs allow two wavefronts per SIMD, eight per CU).  resolve: one count per wavefront
    lds = {"cfhip_inflate_decode_kernel": lambda v: v == 4*(4096 + 64) + 2722 + 674 + 392 + 340 + 128 + 88,
           "cfhip_inflate_resolve_kernel": lambda v: v == 16,
           "cfhip_inflate_fold_kernel": lambda v: v == 3*64*4}
    vgpr = {"cfhip_inflate_decode_kernel": 256}
    for name in KERNELS:
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == 1, (name, sorted(found))
        (k, v), = found.items()
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
        assert lds.get(name, lambda x: x == 0)(v["lds"]), (k, v)
        assert v["vgpr"] <= vgpr.get(name, 64), (k, v)
    build.check_no_vector_spills()
