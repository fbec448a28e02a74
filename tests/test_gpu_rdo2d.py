"""The rate-distortion pass with copies from the block row above on the GPU (cfhip_rdo2d_kernel, csrc/rdo.hip) against
its definition, tests/rdo2d_ref.py: payloads byte for byte and statistics equal, for every row of the table, at the
widths and heights where the kernel takes another path (the first block, the reach of dx, the lookback L, a tile and
its neighbours in both directions), a partial edge, the three pixel types, a mask, a cap, in place, unaligned
payloads, the window, and a mip chain as one batched call."""
import ctypes

import numpy as np
import pytest

import rdo2d_ref
import rdo_ref
from cuttlefish_amd import Alpha, Format, Quality, Texture, Type, api, synth

pytestmark = pytest.mark.gpu

ROWS = sorted(rdo_ref.TABLE)
IDS = [Format(f).name for f, _ in ROWS]
SEG, L, R = rdo_ref.SEG, rdo_ref.L, rdo2d_ref.TILE_ROWS
WIDTHS = (1, 4, 5, L + 1, SEG - 1, SEG, SEG + 1, 2*SEG + 5)          # blocks
HEIGHTS = (1, 2, R, R + 1, 2*R + 1)                                  # block rows
LAM = 8.0
ALL = (True,)*4


def _encode(ctx, images, fmt, typ):
    return ctx.encode(images, api.make_params(fmt, typ, Quality.Lowest))


def _twin(p, im, fmt, typ, lam=LAM, **kw):
    kw = {"max_sse_increase": None, "mask": ALL, **kw}
    return rdo2d_ref.rdo2d(p, im, fmt, typ, lam, kw.pop("max_sse_increase"), kw.pop("mask"), True, **kw)


def _check(got, want, what):
    (out, st), (ref, ref_st) = got, want
    assert np.array_equal(out, ref), (what, int((out != ref).sum()))
    assert st == ref_st, (what, st, ref_st)


def _floats(img, dtype):
    """the image as floats that quantise to other values than img/255 here and there: out of range, NaN, ties"""
    f = img.astype(np.float32)/np.float32(255)
    f[0, 0] = (-0.25, 1.5, np.nan, 0.5)
    f[-1, -1, :3] = np.float32(100.5/255)
    return f.astype(dtype)


@pytest.mark.parametrize("fmt,typ", ROWS, ids=IDS)
def test_shapes_equal_the_twin(gpu_ctx, fmt, typ):
    sizes = [(4*w, 4*r) for w in WIDTHS for r in HEIGHTS] + [(4*(SEG + 1) - 3, 4*R + 1)]
    images = [synth.photo(w, h, seed=fmt + i) for i, (w, h) in enumerate(sizes)]
    plain = _encode(gpu_ctx, images, fmt, typ)
    outs, stats = gpu_ctx.rdo(plain, images, fmt, typ, LAM, row_above=True)
    assert gpu_ctx.last_kernel_name() == "cfhip_rdo2d_kernel"
    for p, im, o, st, size in zip(plain, images, outs, stats, sizes):
        _check((o, st), _twin(p, im, fmt, typ), size)
    # somewhere a block copies from above: the plain pass returns other bytes
    left, _ = gpu_ctx.rdo(plain, images, fmt, typ, LAM)
    assert gpu_ctx.last_kernel_name() == "cfhip_rdo_kernel"
    assert any(not np.array_equal(a, b) for a, b in zip(outs, left))
    # a surface of one block row has no row above
    assert all(np.array_equal(a, b) for a, b, (_, h) in zip(outs, left, sizes) if h == 4)
    # a surface alone returns what it returns in the batch
    one, one_st = gpu_ctx.rdo(plain[-1:], images[-1:], fmt, typ, LAM, row_above=True)
    assert np.array_equal(one[0], outs[-1]) and one_st[0] == stats[-1]


@pytest.mark.parametrize("fmt,typ", ROWS, ids=IDS)
def test_pixel_types_mask_and_cap(gpu_ctx, fmt, typ):
    img = synth.photo(4*(L + 6) - 1, 10, seed=fmt)
    plain = _encode(gpu_ctx, [img], fmt, typ)[0]
    mask = (True, False, True, True) if fmt != rdo_ref.BC4 else (True, True, False, True)
    seen = set()
    for src in (img, _floats(img, np.float32), _floats(img, np.float16)):
        for kw in (dict(), dict(mask=mask), dict(max_sse_increase=40), dict(max_sse_increase=0, mask=mask)):
            outs, stats = gpu_ctx.rdo([plain], [src], fmt, typ, LAM, row_above=True, **kw)
            _check((outs[0], stats[0]), _twin(plain, src, fmt, typ, **kw), (src.dtype, kw))
            seen.add(outs[0].tobytes())
    # a cap of 0 forbids what the free pass does somewhere
    assert len(seen) >= 2
    # no channel compared: every distortion is 0 and the cheapest candidate wins everywhere it exists
    outs, stats = gpu_ctx.rdo([plain], [img], fmt, typ, LAM, mask=(False,)*4, row_above=True)
    _check((outs[0], stats[0]), _twin(plain, img, fmt, typ, mask=(False,)*4), "no channel")
    assert stats[0]["sse_before"] == stats[0]["sse_after"] == 0


@pytest.mark.parametrize("fmt,typ", ROWS, ids=IDS)
def test_in_place_and_unaligned_on_the_device(gpu_ctx, fmt, typ):
    import torch
    sizes = [(4*(2*SEG + 5), 4*(R + 1)), (4*(L + 1) - 2, 7)]
    images = [synth.photo(w, h, seed=3*fmt + i) for i, (w, h) in enumerate(sizes)]
    plain = _encode(gpu_ctx, images, fmt, typ)
    want = [_twin(p, im, fmt, typ) for p, im in zip(plain, images)]
    size = ctypes.sizeof(api.RdoStats)
    tex = [torch.from_numpy(im).cuda() for im in images]
    for shift, in_place in ((0, True), (0, False), (3, True), (3, False)):
        # shift 3: neither payload is aligned to a block, so blocks travel byte by byte
        src = [torch.zeros(p.size + 16, dtype=torch.uint8, device="cuda") for p in plain]
        for s, p in zip(src, plain):
            s[shift:shift + p.size] = torch.from_numpy(p).cuda()
        dst = src if in_place else [torch.zeros_like(s) for s in src]
        stats = torch.full((len(plain)*size,), 0xAB, dtype=torch.uint8, device="cuda")      # the call clears them
        torch.cuda.synchronize()                 # torch filled the buffers on its own stream
        gpu_ctx.rdo_device([dict(blocks=s.data_ptr() + shift, out=d.data_ptr() + shift, out_capacity=p.size,
                                 pixels=t.data_ptr(), pixel_type=0, width=im.shape[1], height=im.shape[0],
                                 row_pitch_bytes=im.shape[1]*4)
                            for s, d, p, t, im in zip(src, dst, plain, tex, images)],
                           fmt, typ, LAM, stats.data_ptr(), row_above=True)
        raw = stats.cpu().numpy().tobytes()
        for i, (d, p) in enumerate(zip(dst, plain)):
            host = d.cpu().numpy()
            st = api.RdoStats.from_buffer_copy(raw[i*size:(i + 1)*size]).as_dict()
            _check((host[shift:shift + p.size], st), want[i], (shift, in_place, i))
            # nothing is written outside the payload
            assert not host[:shift].any() and not host[shift + p.size:].any()
            if not in_place:
                assert np.array_equal(src[i].cpu().numpy()[shift:shift + p.size], p)


@pytest.mark.parametrize("fmt,typ", ROWS, ids=IDS)
def test_mip_chain_is_one_launch(gpu_ctx, fmt, typ):
    images = [synth.photo(s, s, seed=fmt + s) for s in (64, 32, 16, 8, 4, 2, 1)]
    plain = _encode(gpu_ctx, images, fmt, typ)
    gpu_ctx.profile_begin()
    outs, stats = gpu_ctx.rdo(plain, images, fmt, typ, LAM, row_above=True)
    _, launches = gpu_ctx.profile_end()
    assert launches == 1 and gpu_ctx.last_kernel_name() == "cfhip_rdo2d_kernel"
    for p, im, o, st in zip(plain, images, outs, stats):
        _check((o, st), _twin(p, im, fmt, typ), im.shape)
    bits = 8*rdo_ref.TABLE[(fmt, typ)][0]
    assert stats[0]["blocks_changed"] > 0 and stats[-1] == dict(
        blocks=1, blocks_changed=0, sse_before=stats[-1]["sse_before"], sse_after=stats[-1]["sse_before"],
        bits_before=bits, bits_after=bits)


def test_window_decides_per_surface(gpu_ctx):
    # (40 + 4) x 8 bytes lie outside a window of 256, (20 + 4) x 8 inside: both kinds share the launch
    fmt, typ = Format.BC1_RGB, Type.UNorm
    images = [synth.photo(160, 36, seed=1), synth.photo(80, 36, seed=2)]
    plain = _encode(gpu_ctx, images, fmt, typ)
    outs, stats = gpu_ctx.rdo(plain, images, fmt, typ, LAM, row_above=True, window_bytes=256)
    assert gpu_ctx.last_kernel_name() == "cfhip_rdo2d_kernel"
    left, left_st = gpu_ctx.rdo(plain, images, fmt, typ, LAM)
    _check((outs[0], stats[0]), rdo_ref.rdo(plain[0], images[0], fmt, typ, LAM), "outside")
    _check((outs[0], stats[0]), (left[0], left_st[0]), "the plain pass")
    _check((outs[1], stats[1]), _twin(plain[1], images[1], fmt, typ, window_bytes=256), "inside")
    assert not np.array_equal(outs[1], left[1])
    # the edge: 352 bytes hold the row above of the wider surface
    for window, same in ((351, True), (352, False)):
        o, st = gpu_ctx.rdo(plain[:1], images[:1], fmt, typ, LAM, row_above=True, window_bytes=window)
        _check((o[0], st[0]), _twin(plain[0], images[0], fmt, typ, window_bytes=window), window)
        assert np.array_equal(o[0], left[0]) == same


def test_routing_and_identical_calls(gpu_ctx):
    images = [synth.photo(4*(2*SEG + 5), 4*(R + 3), seed=5), synth.photo(40, 40, seed=6)]
    plain = _encode(gpu_ctx, images, Format.BC7, Type.UNorm)
    # no flag through cfhip_rdo_ex: cfhip_rdo's result from cfhip_rdo's kernel
    old = gpu_ctx.rdo(plain, images, Format.BC7, Type.UNorm, 3.0, max_sse_increase=500)
    ex = gpu_ctx.rdo(plain, images, Format.BC7, Type.UNorm, 3.0, max_sse_increase=500, window_bytes=32768)
    assert gpu_ctx.last_kernel_name() == "cfhip_rdo_kernel"
    assert all(np.array_equal(x, y) for x, y in zip(old[0], ex[0])) and old[1] == ex[1]
    a = gpu_ctx.rdo(plain, images, Format.BC7, Type.UNorm, 3.0, max_sse_increase=500, row_above=True)
    b = gpu_ctx.rdo(plain, images, Format.BC7, Type.UNorm, 3.0, max_sse_increase=500, row_above=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]
    assert not any(np.array_equal(x, y) for x, y in zip(a[0], old[0]))
    # no block of the result is in the reserved mode, and the decoder counts no error block
    for out, im in zip(a[0], images):
        assert out.reshape(-1, 16)[:, 0].all()
        assert gpu_ctx.decode(out, Format.BC7, Type.UNorm, im.shape[1], im.shape[0])[1] == 0


def _texture(w, h, mips, dtype, seed):
    t = Texture(w, h, mip_levels=mips)
    for m in range(mips):
        im = synth.photo(t.width(m), t.height(m), seed=seed + m)
        assert t.set_image(im if dtype == np.uint8 else _floats(im, dtype), m)
    return t


@pytest.mark.parametrize("fmt,dtype,kw", [
    (Format.BC1_RGB, np.uint8, {}),
    (Format.BC3, np.float32, dict(max_sse_increase=60)),
    (Format.BC7, np.float16, dict(alpha_type=Alpha.None_, color_mask=(True, False, True, True))),
], ids=["bc1-u8", "bc3-f32-cap", "bc7-f16-masked"])
def test_convert_rdo_equals_convert_then_the_twin(fmt, dtype, kw):
    w, h, mips = 4*(SEG + 2) - 1, 4*(R + 2), 4
    plain, fused, source = (_texture(w, h, mips, dtype, int(fmt)) for _ in range(3))
    conv = {k: v for k, v in kw.items() if k != "max_sse_increase"}
    assert plain.convert(fmt, Type.UNorm, Quality.Low, **conv)
    assert fused.convert_rdo(fmt, Type.UNorm, Quality.Low, rdo_lambda=LAM, row_above=True, **kw)
    assert fused.converted() and (fused.format(), fused.type()) == (fmt, Type.UNorm)
    mask = list(kw.get("color_mask", ALL))
    if kw.get("alpha_type") == Alpha.None_ or not Texture.has_alpha(fmt):
        mask[3] = False
    stats = fused.rdo_stats()
    assert len(stats) == mips
    for m in range(mips):
        src = source.get_image(m)
        src = src.astype(np.float32) if src.dtype == np.float16 else src          # convert() widens halves
        want, want_st = _twin(plain.data(m), src, fmt, Type.UNorm, mask=mask, max_sse_increase=kw.get("max_sse_increase"))
        assert np.array_equal(fused.data(m), want), m
        assert stats[m] == want_st, m
        left, _ = rdo_ref.rdo(plain.data(m), src, fmt, Type.UNorm, LAM, mask=mask,
                              max_sse_increase=kw.get("max_sse_increase"))
        assert m > 0 or not np.array_equal(left, want)
