"""The rate-distortion pass to a target ratio on the GPU (cfhip_rdo_target*) against its definition,
tests/rdo_target_ref.py: the chosen lambda, the trials, the estimates, the payload bytes and the statistics, for BC1
and BC7, a surface of whole segments and a ragged one, two surfaces in one call, with and without the row above, in
place and out of place on the device, the target no lambda reaches, and Texture.convert_rdo(target_ratio=...)."""
import ctypes

import numpy as np
import pytest

import lzsize_ref
import rdo_target_ref
from cuttlefish_amd import Format, Quality, Texture, Type, api, synth

pytestmark = pytest.mark.gpu

FORMATS = [Format.BC1_RGB, Format.BC7]
LAM = 32.0


def _encode(ctx, images, fmt):
    return ctx.encode(images, api.make_params(fmt, Type.UNorm, Quality.Low))


def _check(got, want, what):
    outs, stats, res = got
    ref, ref_stats, ref_res = want
    assert res == ref_res, (what, res, ref_res)
    assert all(np.array_equal(a, b) for a, b in zip(outs, ref)), what
    assert stats == ref_stats, what


@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
@pytest.mark.parametrize("size", [(256, 64), (100, 36)], ids=["256x64", "100x36"])
def test_one_surface_equals_the_twin(gpu_ctx, fmt, size):
    img = synth.photo(size[0], size[1], seed=int(fmt))
    plain = _encode(gpu_ctx, [img], fmt)
    want = rdo_target_ref.rdo_target(plain, [img], fmt, Type.UNorm, 0.9, LAM)
    got = gpu_ctx.rdo_target(plain, [img], fmt, Type.UNorm, 0.9, LAM)
    _check(got, want, (fmt, size))
    res = got[2]
    assert res["est_bytes_plain"] == lzsize_ref.lz_size(plain)["est_bytes"]
    assert res["est_bytes_final"] == gpu_ctx.lz_size(got[0])["est_bytes"]
    assert res["reached"] == 1 and 1 < res["trials"] <= 10 and 0 < res["lambda16"] <= 512
    # the search's launches are all timed
    assert gpu_ctx.last_kernel_ms() > 0.0


@pytest.mark.parametrize("fmt", FORMATS, ids=[f.name for f in FORMATS])
@pytest.mark.parametrize("row_above", [False, True], ids=["left", "row-above"])
def test_two_surfaces_on_the_device(gpu_ctx, fmt, row_above):
    import torch
    images = [synth.photo(256, 64, seed=int(fmt) + 1), synth.photo(100, 36, seed=int(fmt) + 2)]
    plain = _encode(gpu_ctx, images, fmt)
    kw = dict(max_sse_increase=400, mask=(True, True, False, True))
    want = rdo_target_ref.rdo_target(plain, images, fmt, Type.UNorm, 0.85, LAM, row_above=row_above, **kw)
    _check(gpu_ctx.rdo_target(plain, images, fmt, Type.UNorm, 0.85, LAM, row_above=row_above, **kw), want, "host")
    size = ctypes.sizeof(api.RdoStats)
    tex = [torch.from_numpy(im).cuda() for im in images]
    stream = torch.cuda.Stream()
    for in_place in (True, False):
        src = [torch.from_numpy(p).cuda() for p in plain]
        dst = src if in_place else [torch.zeros_like(s) for s in src]
        stats = torch.full((2*size,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        res = gpu_ctx.rdo_target_device(
            [dict(blocks=s.data_ptr(), out=d.data_ptr(), out_capacity=p.size, pixels=t.data_ptr(), pixel_type=0,
                  width=im.shape[1], height=im.shape[0], row_pitch_bytes=im.shape[1]*4)
             for s, d, p, t, im in zip(src, dst, plain, tex, images)],
            fmt, Type.UNorm, 0.85, LAM, stats.data_ptr(), row_above=row_above,
            stream=0 if in_place else stream.cuda_stream, **kw)
        raw = stats.cpu().numpy().tobytes()
        got_stats = [api.RdoStats.from_buffer_copy(raw[i*size:(i + 1)*size]).as_dict() for i in range(2)]
        _check(([d.cpu().numpy() for d in dst], got_stats, res), want, ("device", in_place))
        if not in_place:
            assert all(np.array_equal(s.cpu().numpy(), p) for s, p in zip(src, plain))


def test_target_out_of_reach(gpu_ctx):
    img = synth.photo(256, 64, seed=77)
    plain = _encode(gpu_ctx, [img], Format.BC7)
    # a ceiling of 1/4: the pass at lambda16 = 4 is all there is
    want = rdo_target_ref.rdo_target(plain, [img], Format.BC7, Type.UNorm, 0.5, 0.25)
    got = gpu_ctx.rdo_target(plain, [img], Format.BC7, Type.UNorm, 0.5, 0.25)
    _check(got, want, "out of reach")
    assert (got[2]["reached"], got[2]["lambda16"], got[2]["trials"]) == (0, 4, 1)
    one, one_stats = gpu_ctx.rdo(plain, [img], Format.BC7, Type.UNorm, 0.25)
    assert np.array_equal(one[0], got[0][0]) and one_stats == got[1]
    # identical calls return identical bytes
    again = gpu_ctx.rdo_target(plain, [img], Format.BC7, Type.UNorm, 0.5, 0.25)
    _check(again, got, "again")


def test_convert_rdo_to_a_target(gpu_ctx):
    fmt, mips = Format.BC7, 8

    def texture():
        t = Texture(128, 128, mip_levels=mips)
        for m in range(mips):
            assert t.set_image(synth.photo(t.width(m), t.height(m), seed=40 + m), m)
        return t
    plain, fused, source = texture(), texture(), texture()
    assert plain.convert(fmt, Type.UNorm, Quality.Low)
    assert fused.convert_rdo(fmt, Type.UNorm, Quality.Low, rdo_lambda=LAM, target_ratio=0.85)
    images = [source.get_image(m) for m in range(mips)]
    want = rdo_target_ref.rdo_target([plain.data(m) for m in range(mips)], images, fmt, Type.UNorm, 0.85, LAM)
    _check(([fused.data(m) for m in range(mips)], fused.rdo_stats(), fused.rdo_target()), want, "texture")
    size = fused.packed_size()
    assert size == lzsize_ref.lz_size(want[0]) and size["est_bytes"] == want[2]["est_bytes_final"]
    assert plain.packed_size()["est_bytes"] == want[2]["est_bytes_plain"]
    assert want[2]["reached"] == 1 and size["est_bytes"] <= 0.85*want[2]["est_bytes_plain"]
    # without a target every call keeps its bytes, and reports no search
    left = texture()
    assert left.convert_rdo(fmt, Type.UNorm, Quality.Low, rdo_lambda=2.0) and left.rdo_target() is None
    ref = gpu_ctx.rdo([plain.data(m) for m in range(mips)], images, fmt, Type.UNorm, 2.0)
    assert all(np.array_equal(left.data(m), ref[0][m]) for m in range(mips)) and left.rdo_stats() == ref[1]
    # any converted format has a packed size
    astc = texture()
    assert astc.convert(Format.ASTC_6x6, Type.UNorm, Quality.Low)
    assert astc.packed_size() == lzsize_ref.lz_size([astc.data(m) for m in range(mips)])
