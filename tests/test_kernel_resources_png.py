"""The PNG writer's kernels in the built code object: no scratch, no spilled vector register, no AGPR, and the LDS each
is written to take (tests/test_kernel_resources_lz4.py reads the LZ4 codec's the same way)."""
import pytest


def test_png_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    # filter: per wavefront 64 pixels of 8 bytes and the words that align them (132 words), and four times five 64-bit
    # sums.  crc: the byte table and one word per wavefront.  final: none
    lds = {"cfhip_png_filter_kernel": 4*132*4 + 4*5*8, "cfhip_png_crc_kernel": 256*4 + 4*4, "cfhip_png_final_kernel": 0}
    want = {"cfhip_png_filter_kernel": 3*4*2, "cfhip_png_crc_kernel": 1, "cfhip_png_final_kernel": 1}
    for name, count in want.items():
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == count, (name, sorted(found))        # source type x channels x depth
        for k, v in found.items():
            assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
            assert v["lds"] == lds[name], (k, v)
            assert v["vgpr"] <= 64, (k, v)
    build.check_no_vector_spills()
