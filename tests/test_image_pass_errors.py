"""The eight image passes of the C ABI without a GPU: for each entry point a table of argument mutations and the exact
bytes cfhip_last_error holds afterwards.  The ABI tests of the passes match substrings; this file pins whole texts and,
with inputs that carry two faults, which one is reported.  A NULL context stands in for the device and host memory
for the surfaces: every call returns before it would touch either, the valid one with "ctx is NULL", reported last.
The texts are the library's from before the passes shared their checks."""
import ctypes

import numpy as np
import pytest

from cuttlefish_amd import api

_MEM = np.zeros(1 << 16, np.uint8)
BASE = (_MEM.ctypes.data + 4095) & ~4095               # offsets below count from a texel-aligned address
U8, F32, F16 = 0, 1, 2                                 # cfhip pixel types: 4, 16 and 8 bytes a texel


def _ptr(off):
    return None if off is None else BASE + off


def _list(offs):
    return None if offs is None else (ctypes.c_void_p*max(len(offs), 1))(*[_ptr(o) for o in offs])


def _coverage(lib, a):
    surf = None
    if a["surfs"] is not None:
        surf = (api.CoverageSurface*max(len(a["surfs"]), 1))()
        for s, (off, pt, w, h, pitch) in zip(surf, a["surfs"]):
            s.pixels, s.pixel_type, s.width, s.height, s.pitch_bytes = _ptr(off), pt, w, h, pitch
    return lib.cfhip_alpha_coverage_device(None, surf, a["count"], a["thr"], a["scale"], _ptr(a["counts"]), None)


def _mip_post(lib, a):
    p = api.MipPostParams(a["flags"], a["thr"])
    return lib.cfhip_mip_post_array_device(None, _list(a["srcs"]), a["layers"], a["pt"], a["w"], a["h"], a["pitch"],
                                           _list(a["levels"]), a["count"], ctypes.byref(p) if a["params"] else None,
                                           _ptr(a["res"]), None)


def _bleed(lib, a):
    p = api.BleedParams(a["flags"], a["thr"], a["maxd"])
    return lib.cfhip_alpha_bleed_array_device(None, _list(a["images"]), a["layers"], a["pt"], a["w"], a["h"], a["pitch"],
                                              ctypes.byref(p) if a["params"] else None, _ptr(a["res"]), None)


def _sdf(lib, a):
    p = api.SdfParams(a["flags"], a["thr"], a["spread"], a["scale"], a["mask"], a["reserved"])
    return lib.cfhip_alpha_sdf_array_device(None, _list(a["src"]), a["layers"], a["spt"], a["w"], a["h"], a["sp"],
                                            _list(a["dst"]), a["dpt"], a["dp"], ctypes.byref(p) if a["params"] else None,
                                            _ptr(a["res"]), None)


def _spec_aa(lib, a):
    p = api.SpecAaParams(a["size"], a["flags"], a["channel"], a["base"], a["vscale"], a["maxv"],
                         (ctypes.c_uint32*2)(*a["reserved"]))
    return lib.cfhip_spec_aa_array_device(None, _list(a["normals"]), a["layers"], a["npt"], a["w"], a["h"], a["np"],
                                          _list(a["rough"]), a["rpt"], a["rp"], _list(a["levels"]), a["count"],
                                          ctypes.byref(p) if a["params"] else None, _ptr(a["res"]), None)


def _equirect(lib, a):
    return lib.cfhip_equirect_to_cube_device(None, _ptr(a["src"]), a["spt"], a["w"], a["h"], a["pitch"], _list(a["faces"]),
                                             a["face"], a["ss"], None)


_GGX = {}


def _table(kind):
    """a level's sample table: "ggx" = 64 real records, "nan" = the same with record 3 spoilt, None = no table"""
    if kind is None:
        return None
    if kind not in _GGX:
        t = api.ggx_sample_table(0.5, 64, 4, 3)
        if kind == "nan":
            t[3, 0] = np.nan
        _GGX[kind] = t
    return _GGX[kind].ctypes.data


def _prefilter(lib, a):
    tabs = None if a["tables"] is None else (ctypes.c_void_p*len(a["tables"]))(*[_table(t) for t in a["tables"]])
    cnt = None if a["samples"] is None else (ctypes.c_uint32*len(a["samples"]))(*a["samples"])
    return lib.cfhip_cube_prefilter_device(None, _list(a["src"]), a["face"], a["L"], _list(a["dst"]), a["K"], tabs, cnt, None)


def _sh9(lib, a):
    return lib.cfhip_cube_sh9_device(None, _list(a["faces"]), a["face"], _ptr(a["res"]), None)


def _but(seq, **at):
    """seq with the elements at the given indices (i0=..., i4=...) replaced"""
    out = list(seq)
    for k, v in at.items():
        out[int(k[1:])] = v
    return out


LEV = [2048, 2304, 2560, 3072, 3328, 3584]             # two layers, levels 1 to 3 of each
FACES = [0, 256, 512, 768, 1024, 1280]
SRC_LEVELS = [256*i for i in range(18)]                # six faces, three levels each
DST_LEVELS = [8192 + 256*i for i in range(12)]         # six faces, two levels each
COV = [(0, U8, 4, 4, 16), (1024, F32, 4, 4, 64)]

# pass -> (the call, its valid arguments, [(the arguments that differ, cfhip_last_error after the call)])
CASES = {
    "alpha_coverage": (_coverage, dict(surfs=COV, count=2, thr=0.5, scale=1.0, counts=4096), [
        (dict(), b"ctx is NULL"),
        (dict(surfs=None), b"alpha_coverage: surfaces is NULL"),
        (dict(counts=None), b"alpha_coverage: counts_device is NULL"),
        (dict(count=0), b"alpha_coverage: count is 0"),
        (dict(thr=0.0), b"alpha_coverage: threshold 0 outside (0, 1]"),
        (dict(thr=1.5), b"alpha_coverage: threshold 1.5 outside (0, 1]"),
        (dict(scale=0.0), b"alpha_coverage: scale 0 is not a positive finite number"),
        (dict(surfs=_but(COV, i1=(None, F32, 4, 4, 64))), b"alpha_coverage: surfaces[1].pixels is NULL"),
        (dict(surfs=_but(COV, i0=(0, U8, 0, 4, 16))), b"alpha_coverage: surfaces[0] has a zero width or height"),
        (dict(surfs=_but(COV, i0=(0, 7, 4, 4, 16))), b"alpha_coverage: surfaces[0]: pixel type 7"),
        (dict(surfs=_but(COV, i0=(0, U8, 4, 4, 15))), b"alpha_coverage: surfaces[0]: pitch_bytes 15 < 16"),
        (dict(surfs=_but(COV, i0=(0, U8, 65536, 32768, 262144))), b"alpha_coverage: surfaces[0]: more than 2^30 texels"),
        (dict(surfs=_but(COV, i1=(1026, F32, 4, 4, 64))),
         b"alpha_coverage: surfaces[1]: pixels or pitch_bytes not aligned to a component"),
        (dict(surfs=_but(COV, i1=(1024, F32, 4, 4, 66))),
         b"alpha_coverage: surfaces[1]: pixels or pitch_bytes not aligned to a component"),
        # two faults
        (dict(surfs=[(2, F32, 4, 4, 64), (None, F32, 4, 4, 64)]),
         b"alpha_coverage: surfaces[0]: pixels or pitch_bytes not aligned to a component"),
        (dict(thr=0.0, surfs=_but(COV, i1=(None, F32, 4, 4, 64))), b"alpha_coverage: threshold 0 outside (0, 1]"),
    ]),
    "mip_post": (_mip_post, dict(srcs=[0, 1024], layers=2, pt=F32, w=8, h=4, pitch=128, levels=LEV, count=4, flags=1,
                                 thr=0.5, params=True, res=8192), [
        (dict(), b"ctx is NULL"),
        (dict(flags=2, res=None), b"ctx is NULL"),
        (dict(params=False), b"mip_post: params is NULL"),
        (dict(srcs=None), b"mip_post: srcs is NULL"),
        (dict(levels=None), b"mip_post: levels is NULL"),
        (dict(layers=0), b"mip_post: layers is 0 (1 to 65535 per call)"),
        (dict(layers=65536), b"mip_post: layers is 65536 (1 to 65535 per call)"),
        (dict(w=0), b"mip_post: a zero width or height (0x4)"),
        (dict(pt=3), b"mip_post: src_pixel_type 3"),
        (dict(count=1), b"mip_post: levels_count is 1, a chain to repair has 2 to 4 levels at 8x4"),
        (dict(count=5), b"mip_post: levels_count is 5, a chain to repair has 2 to 4 levels at 8x4"),
        (dict(flags=0), b"mip_post: params->flags 0x0: none or unknown"),
        (dict(flags=9), b"mip_post: params->flags 0x9: none or unknown"),
        (dict(flags=4), b"mip_post: params->flags: SIGNED_NORMALS without NORMALIZE"),
        (dict(thr=0.0), b"mip_post: params->alpha_threshold 0 outside (0, 1]"),
        (dict(pitch=127), b"mip_post: src_pitch_bytes 127 < 128, a row"),
        (dict(res=None), b"mip_post: results_device is NULL under COVERAGE"),
        (dict(w=65536, h=32768, pitch=1 << 20, count=2), b"mip_post: more than 2^30 texels in level 0"),
        (dict(srcs=[0, None]), b"mip_post: srcs[1] is NULL"),
        (dict(srcs=[0, 1026]), b"mip_post: srcs[1] or src_pitch_bytes not aligned to a component"),
        (dict(levels=_but(LEV, i4=None)), b"mip_post: levels[4] (layer 1, level 2) is NULL"),
        (dict(levels=_but(LEV, i0=2052)), b"mip_post: levels[0] is not aligned to a texel (16 bytes)"),
        # two faults: the layers' loop takes a layer's source, then its levels
        (dict(levels=_but(LEV, i0=None), srcs=[0, None]), b"mip_post: levels[0] (layer 0, level 1) is NULL"),
        (dict(levels=_but(LEV, i3=None), srcs=[0, None]), b"mip_post: srcs[1] is NULL"),
        (dict(pitch=127, flags=9), b"mip_post: params->flags 0x9: none or unknown"),
    ]),
    "alpha_bleed": (_bleed, dict(images=[0, 1024], layers=2, pt=U8, w=8, h=8, pitch=32, flags=3, thr=0.0, maxd=0,
                                 params=True, res=8192), [
        (dict(), b"ctx is NULL"),
        (dict(res=None), b"ctx is NULL"),
        (dict(params=False), b"alpha_bleed: params is NULL"),
        (dict(images=None), b"alpha_bleed: images is NULL"),
        (dict(layers=0), b"alpha_bleed: layers is 0 (1 to 65535 per call)"),
        (dict(w=32769), b"alpha_bleed: width and height are 1 to 32768 each, not 32769x8"),
        (dict(h=0), b"alpha_bleed: width and height are 1 to 32768 each, not 8x0"),
        (dict(pt=3), b"alpha_bleed: pixel_type 3"),
        (dict(flags=4), b"alpha_bleed: params->flags 0x4: unknown"),
        (dict(thr=1.0), b"alpha_bleed: params->alpha_threshold 1 outside [0, 1)"),
        (dict(thr=-0.25), b"alpha_bleed: params->alpha_threshold -0.25 outside [0, 1)"),
        (dict(maxd=65536), b"alpha_bleed: params->max_distance 65536 above 65535"),
        (dict(pitch=31), b"alpha_bleed: pitch_bytes 31 < 32, a row"),
        (dict(pt=F16, pitch=65), b"alpha_bleed: pitch_bytes 65 not aligned to a component (2 bytes)"),
        (dict(layers=3, w=32768, h=32768, pitch=131072), b"alpha_bleed: more than 2^31 texels in one call"),
        (dict(images=[0, None]), b"alpha_bleed: images[1] is NULL"),
        (dict(pt=F32, pitch=128, images=[0, 1026]), b"alpha_bleed: images[1] not aligned to a component (4 bytes)"),
        # two faults
        (dict(pt=F32, pitch=128, images=[2, None]), b"alpha_bleed: images[0] not aligned to a component (4 bytes)"),
        (dict(pitch=31, thr=1.0), b"alpha_bleed: params->alpha_threshold 1 outside [0, 1)"),
    ]),
    "alpha_sdf": (_sdf, dict(src=[0, 1024], layers=2, spt=F32, w=8, h=8, sp=128, dst=[2048, 3072], dpt=F16, dp=32, flags=3,
                             thr=0.5, spread=4, scale=2, mask=8, reserved=0, params=True, res=8192), [
        (dict(), b"ctx is NULL"),
        (dict(res=None, scale=1, dp=128, dpt=F32, dst=[0, 1024]), b"ctx is NULL"),
        (dict(params=False), b"alpha_sdf: params is NULL"),
        (dict(src=None), b"alpha_sdf: src is NULL"),
        (dict(dst=None), b"alpha_sdf: dst is NULL"),
        (dict(layers=65536), b"alpha_sdf: layers is 65536 (1 to 65535 per call)"),
        (dict(w=0), b"alpha_sdf: width and height are 1 to 32768 each, not 0x8"),
        (dict(spt=-1), b"alpha_sdf: src_pixel_type -1"),
        (dict(dpt=3), b"alpha_sdf: dst_pixel_type 3"),
        (dict(flags=4), b"alpha_sdf: params->flags 0x4: unknown"),
        (dict(thr=1.0), b"alpha_sdf: params->alpha_threshold 1 outside [0, 1)"),
        (dict(spread=127), b"alpha_sdf: params->spread 127 outside 1 to 126"),
        (dict(scale=3), b"alpha_sdf: params->scale 3 is not 1, 2, 4, 8 or 16"),
        (dict(mask=16), b"alpha_sdf: params->channel_mask 0x10 outside 1 to 15"),
        (dict(reserved=1), b"alpha_sdf: params->reserved is 1, not 0"),
        (dict(w=9, sp=144), b"alpha_sdf: 9x8 is not a multiple of the scale 2"),
        (dict(sp=127), b"alpha_sdf: src_pitch_bytes 127 < 128, a row"),
        (dict(sp=130), b"alpha_sdf: src_pitch_bytes 130 not aligned to a component (4 bytes)"),
        (dict(dp=31), b"alpha_sdf: dst_pitch_bytes 31 < 32, a row"),
        (dict(dp=33), b"alpha_sdf: dst_pitch_bytes 33 not aligned to a component (2 bytes)"),
        (dict(layers=3, w=32768, h=32768, sp=1 << 19, dp=1 << 17), b"alpha_sdf: more than 2^31 texels in one call"),
        (dict(src=[0, None]), b"alpha_sdf: src[1] is NULL"),
        (dict(dst=[2048, None]), b"alpha_sdf: dst[1] is NULL"),
        (dict(src=[2, 1024]), b"alpha_sdf: src[0] not aligned to a component (4 bytes)"),
        (dict(dst=[2048, 3073]), b"alpha_sdf: dst[1] not aligned to a component (2 bytes)"),
        (dict(dst=[2048, 1024]), b"alpha_sdf: dst[1] equals src[1]: in place needs scale 1 and equal pixel types"),
        # two faults: the layers' loop takes both lists of a layer before the next layer
        (dict(dst=[None, 3072], src=[0, None]), b"alpha_sdf: dst[0] is NULL"),
        (dict(src=[2, 1024], dst=[None, 3072]), b"alpha_sdf: dst[0] is NULL"),
        (dict(dp=31, sp=130), b"alpha_sdf: src_pitch_bytes 130 not aligned to a component (4 bytes)"),
    ]),
    "spec_aa": (_spec_aa, dict(normals=[0, 1024], layers=2, npt=F16, w=8, h=4, np=64, rough=[4096, 5120], rpt=F32, rp=128,
                               levels=LEV, count=4, size=32, flags=7, channel=1, base=0.5, vscale=1.0, maxv=1.0,
                               reserved=(0, 0), params=True, res=8192), [
        (dict(), b"ctx is NULL"),
        (dict(rough=None, rpt=99, rp=0, res=None), b"ctx is NULL"),
        (dict(params=False), b"spec_aa: params is NULL"),
        (dict(size=24), b"spec_aa: params->struct_size is 24, not 32"),
        (dict(normals=None), b"spec_aa: normals is NULL"),
        (dict(levels=None), b"spec_aa: levels is NULL"),
        (dict(layers=0), b"spec_aa: layers is 0 (1 to 65535 per call)"),
        (dict(h=32769), b"spec_aa: width and height are 1 to 32768 each, not 8x32769"),
        (dict(npt=3), b"spec_aa: normal_pixel_type 3"),
        (dict(rpt=3), b"spec_aa: rough_pixel_type 3"),
        (dict(flags=8), b"spec_aa: params->flags 0x8: unknown"),
        (dict(channel=4), b"spec_aa: params->channel 4 above 3"),
        (dict(base=1.5), b"spec_aa: params->base_roughness 1.5 outside [0, 1]"),
        (dict(vscale=-0.5), b"spec_aa: params->variance_scale -0.5 is negative or not finite"),
        (dict(maxv=-0.5), b"spec_aa: params->max_variance -0.5 is negative or not finite"),
        (dict(reserved=(0, 1)), b"spec_aa: params->reserved is not 0"),
        (dict(count=1), b"spec_aa: levels_count 1 outside 2 to 4, the chain of 8x4"),
        (dict(count=5), b"spec_aa: levels_count 5 outside 2 to 4, the chain of 8x4"),
        (dict(np=63), b"spec_aa: normal_pitch_bytes 63 < 64, a row"),
        (dict(np=68), b"spec_aa: normal_pitch_bytes 68 not aligned to a texel (8 bytes)"),
        (dict(rp=127), b"spec_aa: rough_pitch_bytes 127 < 128, a row"),
        (dict(rp=130), b"spec_aa: rough_pitch_bytes 130 not aligned to a component (4 bytes)"),
        (dict(normals=[0, None]), b"spec_aa: normals[1] is NULL"),
        (dict(normals=[0, 1028]), b"spec_aa: normals[1] not aligned to a texel (8 bytes)"),
        (dict(rough=[None, 5120]), b"spec_aa: rough0[0] is NULL"),
        (dict(rough=[4096, 5122]), b"spec_aa: rough0[1] not aligned to a component (4 bytes)"),
        (dict(levels=_but(LEV, i5=None)), b"spec_aa: levels[5] (layer 1, level 3) is NULL"),
        (dict(levels=_but(LEV, i2=2564)), b"spec_aa: levels[2] is not aligned to a texel (16 bytes)"),
        # two faults: the layers' loop takes a layer's normals, its roughness, then its levels
        (dict(levels=_but(LEV, i0=None), normals=[0, None]), b"spec_aa: levels[0] (layer 0, level 1) is NULL"),
        (dict(rough=[4098, 5120], normals=[0, None]), b"spec_aa: rough0[0] not aligned to a component (4 bytes)"),
        (dict(rp=127, np=68), b"spec_aa: normal_pitch_bytes 68 not aligned to a texel (8 bytes)"),
    ]),
    "equirect_to_cube": (_equirect, dict(src=4096, spt=F16, w=8, h=4, pitch=64, faces=FACES, face=2, ss=2), [
        (dict(), b"ctx is NULL"),
        (dict(src=None), b"equirect_to_cube: src is NULL"),
        (dict(w=1), b"equirect_to_cube: width is 2 to 32768 and height 1 to 32768, not 1x4"),
        (dict(spt=3), b"equirect_to_cube: src_pixel_type 3"),
        (dict(pitch=63), b"equirect_to_cube: src_pitch_bytes 63 < 64, a row"),
        (dict(pitch=65), b"equirect_to_cube: src_pitch_bytes 65 not aligned to a component (2 bytes)"),
        (dict(src=4097), b"equirect_to_cube: src not aligned to a component (2 bytes)"),
        (dict(ss=3), b"equirect_to_cube: supersample 3 is not 1, 2 or 4"),
        (dict(faces=None), b"equirect_to_cube: faces is NULL"),
        (dict(face=8193), b"equirect_to_cube: face_size is 1 to 8192, not 8193"),
        (dict(faces=_but(FACES, i5=None)), b"equirect_to_cube: faces[5] is NULL"),
        (dict(faces=_but(FACES, i2=516)), b"equirect_to_cube: faces[2] not aligned to a texel (16 bytes)"),
        (dict(faces=_but(FACES, i3=4096)), b"equirect_to_cube: faces[3] equals src"),
        # two faults
        (dict(faces=_but(FACES, i1=260, i0=None)), b"equirect_to_cube: faces[0] is NULL"),
        (dict(faces=_but(FACES, i1=4096, i4=None)), b"equirect_to_cube: faces[4] is NULL"),
        (dict(ss=3, faces=None), b"equirect_to_cube: supersample 3 is not 1, 2 or 4"),
    ]),
    "cube_prefilter": (_prefilter, dict(src=SRC_LEVELS, face=4, L=3, dst=DST_LEVELS, K=2, tables=[None, "ggx"],
                                        samples=[0, 64]), [
        (dict(), b"ctx is NULL"),
        (dict(src=None), b"cube_prefilter: src_levels is NULL"),
        (dict(dst=None), b"cube_prefilter: dst_levels is NULL"),
        (dict(tables=None), b"cube_prefilter: tables is NULL"),
        (dict(samples=None), b"cube_prefilter: table_samples is NULL"),
        (dict(face=0), b"cube_prefilter: face_size is 1 to 8192, not 0"),
        (dict(L=4), b"cube_prefilter: source_levels is 1 to 3 for a face of 4, not 4"),
        (dict(K=0), b"cube_prefilter: dst_count is 1 to 3 for a face of 4, not 0"),
        (dict(src=_but(SRC_LEVELS, i7=None)), b"cube_prefilter: src_levels[2][1] is NULL"),
        (dict(src=_but(SRC_LEVELS, i17=4356)), b"cube_prefilter: src_levels[5][2] not aligned to a texel (16 bytes)"),
        (dict(dst=_but(DST_LEVELS, i3=None)), b"cube_prefilter: dst_levels[1][1] is NULL"),
        (dict(dst=_but(DST_LEVELS, i0=8196)), b"cube_prefilter: dst_levels[0][0] not aligned to a texel (16 bytes)"),
        (dict(dst=_but(DST_LEVELS, i2=1024)), b"cube_prefilter: dst_levels[1][0] equals src_levels[1][1]"),
        (dict(L=1, src=SRC_LEVELS[:6], samples=[0, 0]),
         b"cube_prefilter: table_samples[1] is 0, a copy, but there are 1 source levels"),
        (dict(samples=[0, 96]), b"cube_prefilter: table_samples[1] is 96, not 0 or a multiple of 64 from 64 to 4096"),
        (dict(tables=[None, None]), b"cube_prefilter: tables[1] is NULL"),
        (dict(tables=[None, "nan"]), b"cube_prefilter: tables[1][3] is not finite with lz >= 0 and 0 <= lod <= 14"),
        # two faults: all of src_levels before any of dst_levels
        (dict(dst=_but(DST_LEVELS, i0=None), src=_but(SRC_LEVELS, i17=None)), b"cube_prefilter: src_levels[5][2] is NULL"),
        (dict(dst=_but(DST_LEVELS, i0=0, i1=None)), b"cube_prefilter: dst_levels[0][0] equals src_levels[0][0]"),
        (dict(samples=[0, 96], dst=_but(DST_LEVELS, i11=None)), b"cube_prefilter: dst_levels[5][1] is NULL"),
    ]),
    "cube_sh9": (_sh9, dict(faces=FACES, face=2, res=4096), [
        (dict(), b"ctx is NULL"),
        (dict(faces=None), b"cube_sh9: faces is NULL"),
        (dict(face=0), b"cube_sh9: face_size is 1 to 8192, not 0"),
        (dict(faces=_but(FACES, i0=None)), b"cube_sh9: faces[0] is NULL"),
        (dict(faces=_but(FACES, i4=1032)), b"cube_sh9: faces[4] not aligned to a texel (16 bytes)"),
        (dict(res=None), b"cube_sh9: result_device is NULL"),
        (dict(res=4100), b"cube_sh9: result_device not aligned to 8 bytes"),
        # two faults
        (dict(res=None, faces=_but(FACES, i5=None)), b"cube_sh9: faces[5] is NULL"),
        (dict(faces=_but(FACES, i3=None, i2=520)), b"cube_sh9: faces[2] not aligned to a texel (16 bytes)"),
    ]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_argument_error_has_its_text_and_its_turn(hip_lib, name):
    call, valid, rows = CASES[name]
    for change, text in rows:
        rc = call(hip_lib, dict(valid, **change))
        got = hip_lib.cfhip_last_error(None)
        print(name, change, got)
        assert rc == api.E_INVALID, (change, rc)
        assert got == text, change
    assert not _MEM.any()
