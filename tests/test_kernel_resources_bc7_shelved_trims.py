"""The twelfth step of DESIGN.md section 4.1 (mode 6's exchange once per row under the execution mask, part B's extremes
by three-operand minimum / maximum, the error from the key sum, the refit sums unrolled) keeps every BC7 instance inside
its limits, read from the code objects inside the built library (no GPU needed): all 20 instances
<PIX, UNITW, WIDE, LEVEL> without scratch, vector spill or AGPRs; the linear-metric builds in at most 128 VGPRs (4 waves
per SIMD), the perceptual ones in at most 168 (3 waves); LDS exactly 38 784 / 40 832 B, four workgroups per CU.  The items
that could not hold these limits beside the others (the texel search as straight-line code together with the unrolled
refit sums; phase 1's two partitions in one pass) are not in the tree."""
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


def _disassembly(lib):
    """{kernel name: [opcode, ...]} of the BC7 instances inside the library"""
    import re
    import shutil
    import subprocess
    import tempfile
    from cuttlefish_amd import build
    objdump = os.path.join(build.LLVM_BIN, "llvm-objdump")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cp = shutil.copy(lib, d)
        subprocess.run([objdump, "--offloading", cp], cwd=d, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(d)):
            if "amdgcn" not in f:
                continue
            txt = subprocess.run([objdump, "-d", "--no-show-raw-insn", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in txt.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = m.group(1)
                elif cur and STEM in cur and line.startswith("\t"):
                    out.setdefault(cur, []).append(line.split()[0])
    return out


def test_no_matrix_instruction_inside_the_masked_exchange(instances):
    """Mode 6's half exchange runs under the execution mask of the mode-6 lanes (assign_lsq_lane: `if (m6)` behind a
    row's last MFMA).  A v_mfma inside that region would mis-read the A rows of the lanes switched off, silently: so
    every region that opens by saving the mask and holds the exchange's v_min_i32_dpp must close without one, and every
    linear instance must hold such regions and no exchange outside them."""
    dis = _disassembly(LIB)
    assert len(dis) == 20, sorted(dis)
    for name, ops in sorted(dis.items()):
        if "ELb1ELb" not in name[:45]:
            # the perceptual search is not on the matrix pipe and keeps its exchange per texel, outside any mask
            assert not any(op.startswith("v_mfma") for op in ops), name
            continue
        regions, inside, dpp, mfma = 0, False, 0, 0
        for op in ops:
            if op.startswith("s_and_saveexec"):
                inside, dpp, mfma = True, 0, 0
            elif inside and op.startswith("v_min_i32_dpp"):
                dpp += 1
            elif inside and op.startswith("v_mfma"):
                mfma += 1
            elif inside and op.startswith("s_or_b64"):
                if dpp:
                    assert mfma == 0, "%s: v_mfma inside the masked mode-6 exchange" % name
                    assert dpp == 4, (name, dpp)
                    regions += 1
                inside = False
        # (the only v_min_i32_dpp of a linear instance are the exchange's: all of them lie in such regions)
        assert regions >= 2 and 4*regions == sum(op.startswith("v_min_i32_dpp") for op in ops), (name, regions)
