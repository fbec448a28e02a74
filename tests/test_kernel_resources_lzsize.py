"""The estimator's kernels in the built code object: no scratch, no spilled vector register, no AGPR; the parse kernel's
LDS is one chunk of (L, D) words and one cost block's counters per workgroup of one wavefront, and no other kernel of
the family uses LDS."""
import pytest

import lzsize_ref

KERNELS = ("cfhip_lz_keys_kernel", "cfhip_lz_match_kernel", "cfhip_lz_parse_kernel", "cfhip_lz_cost_kernel",
           "cfhip_lz_final_kernel")


def test_lz_kernels_have_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    for name in KERNELS:
        assert name in build.BLOCK_KERNELS
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == 1, (name, sorted(found))
        (k, v), = found.items()
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
        # 16 KiB of staged L / D and 320 counters: nine workgroups (wavefronts) fit the 160 KiB of a CU
        lds = 4*lzsize_ref.CHUNK + 4*320 if name == "cfhip_lz_parse_kernel" else 0
        assert v["lds"] == lds, (k, v)
        assert v["vgpr"] <= 24, (k, v)          # three register granules: eight wavefronts per SIMD with room to spare
    build.check_no_vector_spills()
