"""The zlib encoder's kernels in the built code object: no scratch, no spilled vector register, no AGPR, and the LDS
each one was designed around (tests/test_kernel_resources_lzsize.py reads the estimator's the same way)."""
import pytest

import lzsize_ref

KERNELS = ("cfhip_deflate_parse_kernel", "cfhip_deflate_adler_kernel", "cfhip_deflate_codes_kernel",
           "cfhip_deflate_lengths_kernel", "cfhip_deflate_offsets_kernel", "cfhip_deflate_emit_kernel",
           "cfhip_deflate_final_kernel")


def test_deflate_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    chunk = lzsize_ref.CHUNK
    # parse: the estimator's; emit: the chunk's words padded by one per 64, a code table and 2000 words of bits --
    # six wavefronts per CU; the code builder: 10.2 KiB for an alphabet of 288
    lds = {"cfhip_deflate_parse_kernel": lambda v: v == 4*chunk + 4*320,
           "cfhip_deflate_emit_kernel": lambda v: v == 4*(chunk + chunk//64) + 4*316 + 4*2000,
           "cfhip_deflate_codes_kernel": lambda v: 0 < v <= 12*1024,
           "cfhip_deflate_lengths_kernel": lambda v: 0 < v <= 8*1024,
           "cfhip_deflate_offsets_kernel": lambda v: v == 3*64*4}
    for name in KERNELS:
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == 1, (name, sorted(found))
        (k, v), = found.items()
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
        assert lds.get(name, lambda x: x == 0)(v["lds"]), (k, v)
        assert v["vgpr"] <= 128, (k, v)
    build.check_no_vector_spills()
