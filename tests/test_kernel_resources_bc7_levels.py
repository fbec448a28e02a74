"""BC7's per-level kernel instances, read from the code objects inside the built library (no GPU needed): all 20
exist -- <PIX, UNITW, WIDE, LEVEL> with levels 0, 1, 2 in the 32-lane layouts and 3, 4 in the wide one -- each
without scratch, vector spill or AGPRs, inside the register budget of its occupancy (128 for the linear-metric
builds at 4 waves, 168 for the perceptual ones at 3) and with the LDS of four workgroups per CU; and the Normal
linear build spills fewer scalars than the 53 of the one body that served Lowest, Low and Normal."""
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


def test_all_twenty_instances_exist(instances):
    want = {_name(pix, unitw, wide, level) for pix in (0, 1) for unitw in (0, 1) for level, wide in LEVEL_WIDE}
    assert len(want) == 20
    assert set(instances) == want, sorted(set(instances) ^ want)


def test_every_instance_keeps_the_register_plan(instances):
    assert instances
    for k, v in instances.items():
        unitw = "ELb1ELb" in k
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["agpr"] == 0, (k, v)
        assert v["vgpr"] <= (128 if unitw else 168), (k, v)
        assert v["lds"] == (38784 if unitw else 40832), (k, v)


def test_normal_spills_fewer_scalars_than_the_shared_body(instances):
    for pix in (0, 1):
        v = instances[_name(pix, 1, 0, 2)]
        assert v["sgpr_spill"] < 53, v
