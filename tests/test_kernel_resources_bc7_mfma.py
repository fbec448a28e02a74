"""The matrix-pipe cross terms and the weight-byte keys of the selector search (tenth step;
assign_lsq_lane in csrc/bc7_encode.hip) keep every BC7 instance
inside its limits, read from the code objects inside the built library (no GPU needed): all 20 instances
<PIX, UNITW, WIDE, LEVEL> without scratch, vector spill or AGPRs; the linear-metric builds in at most 128 VGPRs (4 waves
per SIMD), the perceptual ones in at most 168 (3 waves); LDS at most 40 960 B, four workgroups per CU.  With the weight in
a full byte the four keys of a texel row are live at once, with the MFMA its four result registers; the MFMA's result
stays in vector registers (agpr_count 0) and the linear Normal, High and Highest instances sit at 128 registers."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cuttlefish_amd", "libcuttlefish_hip.so")
STEM = "cfhip_bc7_encode_kernel"
LEVEL_WIDE = ((0, False), (1, False), (2, False), (3, True), (4, True))


def _name(pix, unitw, wide, level):
    return "_Z23%sILi%dELb%dELb%dELi%dEEv10cf_kparams" % (STEM, pix, unitw, wide, level)


@pytest.fixture(scope="module")
def instances():
    from cuttlefish_amd import build
    out = build.kernel_metadata(LIB)
    if out is None:
        pytest.skip("library or ROCm LLVM tools not present")
    return {k: v for k, v in out.items() if STEM in k}


@pytest.mark.parametrize("pix", (0, 1))
@pytest.mark.parametrize("unitw", (1, 0))
@pytest.mark.parametrize("level,wide", LEVEL_WIDE)
def test_instance_stays_inside_its_limits(instances, pix, unitw, level, wide):
    assert len(instances) == 20, sorted(instances)
    v = instances[_name(pix, unitw, int(wide), level)]
    assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["agpr"] == 0, v
    assert v["vgpr"] <= (128 if unitw else 168), v
    assert v["lds"] <= 40960, v
