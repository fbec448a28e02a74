"""The thirteenth step of DESIGN.md section 4.1 (the covariance terms by one fused multiply-add, a fit's weights stored by
and / or on the weight words the fits share) keeps every BC7 instance inside its limits, read from the code objects inside the built
library (no GPU needed): all 20 instances <PIX, UNITW, WIDE, LEVEL> without scratch, vector spill or AGPRs; the
linear-metric builds in at most 128 VGPRs (4 waves per SIMD), the perceptual ones in at most 168 (3 waves); LDS exactly
38 784 / 40 832 B.  Every instance stores its fits' weights with ds_and_b32 / ds_or_b32 and none of them through a flat or global
atomic.  (The step's 1/n item was dropped on its timing, so the table k_inv_n and its loads stay: nothing is asserted
about them.)"""
import os
import shutil
import subprocess

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
    build.build()                     # no-op unless the sources changed since the library was built
    out = build.kernel_metadata(LIB)
    assert out is not None, "the built library and the ROCm LLVM tools (llvm-objdump, llvm-readelf) are needed"
    return {k: v for k, v in out.items() if STEM in k}


@pytest.mark.parametrize("pix", (0, 1))
@pytest.mark.parametrize("unitw", (1, 0))
@pytest.mark.parametrize("level,wide", LEVEL_WIDE)
def test_instance_stays_inside_its_limits(instances, pix, unitw, level, wide):
    assert len(instances) == 20, sorted(instances)
    v = instances[_name(pix, unitw, int(wide), level)]
    assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["agpr"] == 0, v
    assert v["vgpr"] <= (128 if unitw else 168), v
    assert v["lds"] == (38784 if unitw else 40832), v


def _bc7_code_object(tmp):
    """(symbol table, disassembly) of the device code object that holds the BC7 instances"""
    from cuttlefish_amd import build
    objdump = os.path.join(build.LLVM_BIN, "llvm-objdump")
    readelf = os.path.join(build.LLVM_BIN, "llvm-readelf")
    cp = shutil.copy(LIB, tmp)
    subprocess.run([objdump, "--offloading", cp], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for f in sorted(os.listdir(tmp)):
        if "amdgcn" not in f:
            continue
        syms = subprocess.run([readelf, "-s", "--wide", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
        if STEM in syms:
            dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            return syms, dis
    raise AssertionError("no code object with the BC7 instances inside the library")


def test_fits_are_stored_by_lds_and_or(instances, tmp_path):
    syms, dis = _bc7_code_object(str(tmp_path))
    cur, ops = None, {}
    for line in dis.splitlines():
        if line.endswith(">:"):
            cur = line.split("<", 1)[1][:-2]
        elif cur and STEM in cur and line.startswith("\t"):
            ops.setdefault(cur, set()).add(line.split()[0])
    assert len(ops) == 20, sorted(ops)
    for name, o in sorted(ops.items()):
        assert "ds_and_b32" in o and "ds_or_b32" in o, name
        # (the column's address is known to be LDS: no generic or global atomic, no returning form)
        assert not any(op.startswith(("flat_atomic", "global_atomic", "ds_and_rtn", "ds_or_rtn")) for op in o), name
