"""The image-ops entry point of the C-ABI without a GPU: declared and exported, the ctypes struct laid out as the
header's, the kernel's resources, and the order of device calls process_image plans (device replaced by a
recorder)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cuttlefish_hip.h")


def test_header_declares_and_library_exports_image_ops(hip_lib):
    from cuttlefish_amd import api
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "cfhip_image_ops_device" in set(re.findall(r"\b(cfhip_[a-z_0-9]+)\s*\(", text))
    assert "cfhip_image_ops_device" in api.EXPORTS
    assert hasattr(hip_lib, "cfhip_image_ops_device")


def _header_enum(name):
    text = open(HEADER).read()
    body = re.search(r"enum %s \{(.*?)\};" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {k: eval(v) for k, v in re.findall(r"(CFHIP_\w+)\s*=\s*([^,\n]+)", body)}


def test_enums_match_header():
    from cuttlefish_amd import api
    assert _header_enum("cfhip_channel") == {"CFHIP_CHANNEL_" + c.name.rstrip("_").upper(): int(c) for c in api.Channel}
    assert _header_enum("cfhip_rotate") == {"CFHIP_ROTATE_" + r.name: int(r) for r in api.RotateAngle}
    want = {"CFHIP_NORMAL_DEFAULT": 0, "CFHIP_NORMAL_KEEP_SIGN": 1, "CFHIP_NORMAL_WRAP_X": 2, "CFHIP_NORMAL_WRAP_Y": 4}
    assert _header_enum("cfhip_normal_options") == want
    ops = _header_enum("cfhip_image_op")
    names = {"COLOR_SPACE": "ColorSpace", "ROTATE": "Rotate", "GRAYSCALE": "Grayscale", "NORMAL_MAP": "NormalMap",
             "FLIP_X": "FlipX", "FLIP_Y": "FlipY", "SWIZZLE": "Swizzle", "PREMULTIPLY": "PreMultiply"}
    assert ops == {"CFHIP_IMAGE_OP_" + k: int(api.ImageOp[v]) for k, v in names.items()}


def test_struct_layout_matches_header(tmp_path):
    from cuttlefish_amd import api
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in api.ImageOps._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                   '  printf("%%zu\\n", sizeof(cfhip_image_ops));\n%s  return 0;\n}\n' %
                   (HEADER, "".join('  printf("%%zu\\n", offsetof(cfhip_image_ops, %s));\n' % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(api.ImageOps)
    assert got[1:] == [getattr(api.ImageOps, f).offset for f in fields]


def test_image_ops_kernel_has_no_scratch_spill_or_agpr(hip_lib):
    from cuttlefish_amd import build
    meta = build.kernel_metadata()
    if meta is None:
        pytest.skip("ROCm LLVM tools absent")
    ks = {k: v for k, v in meta.items() if "cfhip_image_ops_kernel" in k}
    assert len(ks) == 3, sorted(ks)                 # one per source pixel type
    for k, v in ks.items():
        assert v["scratch"] == 0 and (v["vgpr_spill"] or 0) == 0 and (v["agpr"] or 0) == 0, (k, v)
    assert "cfhip_image_ops_kernel" in build.BLOCK_KERNELS


class _Recorder:
    """stands in for image._Device: records the calls, tracks sizes, moves no pixels"""
    calls = []

    def __init__(self, device_id=0):
        pass

    def upload(self, pixels):
        return (pixels.shape[1], pixels.shape[0])

    def ops(self, buf, ops):
        from cuttlefish_amd.api import ImageOp, RotateAngle
        w, h = buf
        quarter = (ops.ops & ImageOp.Rotate) and ops.rotate not in (RotateAngle.CW180, RotateAngle.CCW180)
        _Recorder.calls.append(("ops", ImageOp(ops.ops), bool(ops.rgbf), ops.src_color_space, ops.normal_options))
        return (h, w) if quarter else (w, h)

    def resize(self, buf, width, height, color_space, filter):
        _Recorder.calls.append(("resize", width, height, int(color_space)))
        return (width, height)

    def download(self, buf):
        w, h = buf
        return np.zeros((h, w, 4), np.float32)


@pytest.fixture
def recorder(monkeypatch):
    from cuttlefish_amd import image
    monkeypatch.setattr(image, "_Device", _Recorder)
    _Recorder.calls = []
    return _Recorder.calls


def _run(src_size, width, height, mip=0, normal=False, typ=0, **kw):
    from cuttlefish_amd import process_image
    img = np.zeros((src_size[1], src_size[0], 4), np.uint8)
    return process_image(img, 1, 0, width, height, mip_level=mip, type=typ,
                         normal_map=(0, 2.0) if normal else None, flip_x=True, grayscale=True, rotate=3, **kw)


def test_plan_without_resize_or_normal_map_is_one_call(recorder):
    from cuttlefish_amd.api import ImageOp as Op
    out = _run((64, 32), 64, 32)
    assert recorder == [("ops", Op.ColorSpace | Op.Rotate | Op.Grayscale | Op.FlipX, False, 1, 0)]
    assert out.shape == (64, 32, 4)                   # rotated by 90 degrees


def test_plan_resize_at_mip_k_without_normal_map(recorder):
    from cuttlefish_amd.api import ImageOp as Op
    _run((64, 32), 64, 32, mip=2)
    assert recorder == [("ops", Op.ColorSpace, False, 1, 0), ("resize", 16, 8, 0),
                        ("ops", Op.Rotate | Op.Grayscale | Op.FlipX, False, 0, 0)]


def test_plan_normal_map_at_mip_0_without_resize(recorder):
    from cuttlefish_amd.api import ImageOp as Op
    _run((64, 32), 64, 32, normal=True)
    assert recorder == [("ops", Op.ColorSpace | Op.Rotate | Op.Grayscale | Op.NormalMap | Op.FlipX, True, 1, 0)]


def test_plan_normal_map_at_mip_0_with_resize(recorder):
    from cuttlefish_amd.api import ImageOp as Op
    _run((100, 50), 64, 32, normal=True)
    assert recorder == [("ops", Op.ColorSpace, False, 1, 0), ("resize", 64, 32, 0),
                        ("ops", Op.Rotate | Op.Grayscale | Op.NormalMap | Op.FlipX, True, 0, 0)]


def test_plan_normal_map_at_mip_k_is_made_full_size_then_resized(recorder):
    from cuttlefish_amd.api import ImageOp as Op
    _run((64, 32), 64, 32, mip=2, normal=True)
    assert recorder == [("ops", Op.ColorSpace | Op.Rotate | Op.Grayscale | Op.NormalMap, False, 1, 0),
                        ("resize", 16, 8, 0), ("ops", Op.FlipX, True, 0, 0)]


def test_plan_two_resizes_and_rgbf_flag_without_other_ops(recorder):
    from cuttlefish_amd import process_image
    from cuttlefish_amd.api import ImageOp as Op
    process_image(np.zeros((50, 100, 4), np.float32), 0, 0, 64, 32, mip_level=1, type=1, normal_map=(2, 1.0))
    # SNorm forces KeepSign (1) on top of WrapX (2); the last call only carries the RGBF flag
    assert recorder == [("resize", 64, 32, 0), ("ops", Op.NormalMap, False, 0, 3), ("resize", 32, 16, 0),
                        ("ops", Op(0), True, 0, 0)]


def test_plan_nothing_to_do_still_converts(recorder):
    from cuttlefish_amd import process_image
    from cuttlefish_amd.api import ImageOp as Op
    out = process_image(np.zeros((8, 8, 4), np.uint8), 0, 0, 8, 8)
    assert recorder == [("ops", Op(0), False, 0, 0)]
    assert out.dtype == np.float32
