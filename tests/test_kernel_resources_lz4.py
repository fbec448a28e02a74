"""The LZ4 codec's kernels in the built code object: no scratch, no spilled vector register, no AGPR, and at most the
160 KiB of LDS a CU has (tests/test_kernel_resources_inflate.py reads the inflater's the same way)."""
import pytest

KERNELS = ("cfhip_lz4_match_kernel", "cfhip_lz4_parse_kernel", "cfhip_lz4_plan_kernel", "cfhip_lz4_offsets_kernel",
           "cfhip_lz4_emit_kernel", "cfhip_lz4_hash_kernel", "cfhip_lz4_final_kernel", "cfhip_lz4_chain_kernel",
           "cfhip_lz4_block_kernel", "cfhip_lz4_dfinal_kernel")


def test_lz4_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # parse: a chunk's 4096 (L, D) words, its at most 1024 match records of two words, one count.  plan: 16 counts, the
    # scan's 256 words, one sum.  hash: one tile of 64 stripes.  block: the stored bytes (65536 + 16), the output
    # (65536), 64 records of five words, the tile, three control words: one workgroup per CU
    lds = {"cfhip_lz4_parse_kernel": 4*4096 + 8*1024 + 4, "cfhip_lz4_plan_kernel": 4*(16 + 256 + 1),
           "cfhip_lz4_hash_kernel": 1024, "cfhip_lz4_block_kernel": 65536 + 16 + 65536 + 64*5*4 + 1024 + 12}
    for name in KERNELS:
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == 1, (name, sorted(found))
        (k, v), = found.items()
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
        assert v["lds"] == lds.get(name, 0) and v["lds"] <= 163840, (k, v)
        assert v["vgpr"] <= 64, (k, v)
    build.check_no_vector_spills()
