"""The rate-distortion pass on the GPU (csrc/rdo.hip) against its definition, tests/rdo_ref.py: payloads byte for
byte and statistics equal, for every row of the table, at the widths where the kernel takes another path (the first
block, the lookback L, a segment and its neighbours), with one and three block rows, a partial edge, the three
pixel types, a mask, a cap, in place, unaligned payloads, and a mip chain as one batched call."""
import ctypes

import numpy as np
import pytest

import rdo_ref
from cuttlefish_amd import Alpha, Format, Quality, Texture, Type, api, synth

pytestmark = pytest.mark.gpu

ROWS = sorted(rdo_ref.TABLE)
IDS = [Format(f).name for f, _ in ROWS]
SEG, L = rdo_ref.SEG, rdo_ref.L
WIDTHS = (1, 2, L, L + 1, SEG - 1, SEG, SEG + 1, 2*SEG + 5)          # blocks
LAM = 8.0


def _encode(ctx, images, fmt, typ):
    return ctx.encode(images, api.make_params(fmt, typ, Quality.Lowest))


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
    sizes = [(4*w, 4*r) for w in WIDTHS for r in (1, 3)] + [(4*(SEG + 1) - 3, 5)]
    images = [synth.photo(w, h, seed=fmt + i) for i, (w, h) in enumerate(sizes)]
    plain = _encode(gpu_ctx, images, fmt, typ)
    outs, stats = gpu_ctx.rdo(plain, images, fmt, typ, LAM)
    changed = 0
    for p, im, o, st, size in zip(plain, images, outs, stats, sizes):
        _check((o, st), rdo_ref.rdo(p, im, fmt, typ, LAM), size)
        changed += st["blocks_changed"]
    assert changed > 0
    # a surface alone returns what it returns in the batch
    one, one_st = gpu_ctx.rdo(plain[-1:], images[-1:], fmt, typ, LAM)
    assert np.array_equal(one[0], outs[-1]) and one_st[0] == stats[-1]


@pytest.mark.parametrize("fmt,typ", ROWS, ids=IDS)
def test_pixel_types_mask_and_cap(gpu_ctx, fmt, typ):
    img = synth.photo(4*(L + 6) - 1, 10, seed=fmt)
    plain = _encode(gpu_ctx, [img], fmt, typ)[0]
    mask = (True, False, True, True) if fmt != rdo_ref.BC4 else (True, True, False, True)
    seen = set()
    for src in (img, _floats(img, np.float32), _floats(img, np.float16)):
        for kw in (dict(), dict(mask=mask), dict(max_sse_increase=40), dict(max_sse_increase=0, mask=mask)):
            outs, stats = gpu_ctx.rdo([plain], [src], fmt, typ, LAM, **kw)
            _check((outs[0], stats[0]), rdo_ref.rdo(plain, src, fmt, typ, LAM, **{"mask": (True,)*4, **kw}),
                   (src.dtype, kw))
            seen.add(outs[0].tobytes())
    # a cap of 0 forbids what the free pass does somewhere
    assert len(seen) >= 2
    # no channel compared: every distortion is 0 and the cheapest candidate wins everywhere it exists
    outs, stats = gpu_ctx.rdo([plain], [img], fmt, typ, LAM, mask=(False,)*4)
    _check((outs[0], stats[0]), rdo_ref.rdo(plain, img, fmt, typ, LAM, mask=(False,)*4), "no channel")
    assert stats[0]["sse_before"] == stats[0]["sse_after"] == 0


@pytest.mark.parametrize("fmt,typ", ROWS, ids=IDS)
def test_in_place_and_unaligned_on_the_device(gpu_ctx, fmt, typ):
    import torch
    sizes = [(4*(2*SEG + 5), 8), (4*(L + 1) - 2, 7)]
    images = [synth.photo(w, h, seed=3*fmt + i) for i, (w, h) in enumerate(sizes)]
    plain = _encode(gpu_ctx, images, fmt, typ)
    want = [rdo_ref.rdo(p, im, fmt, typ, LAM) for p, im in zip(plain, images)]
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
                           fmt, typ, LAM, stats.data_ptr())
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
def test_mip_chain_is_one_batched_call(gpu_ctx, fmt, typ):
    images = [synth.photo(s, s, seed=fmt + s) for s in (64, 32, 16, 8, 4, 2, 1)]
    plain = _encode(gpu_ctx, images, fmt, typ)
    gpu_ctx.profile_begin()
    outs, stats = gpu_ctx.rdo(plain, images, fmt, typ, LAM)
    _, launches = gpu_ctx.profile_end()
    assert launches == 1 and gpu_ctx.last_kernel_name() == "cfhip_rdo_kernel"
    for p, im, o, st in zip(plain, images, outs, stats):
        _check((o, st), rdo_ref.rdo(p, im, fmt, typ, LAM), im.shape)
    assert stats[0]["blocks_changed"] > 0 and stats[-1] == dict(
        blocks=1, blocks_changed=0, sse_before=stats[-1]["sse_before"], sse_after=stats[-1]["sse_before"],
        bits_before=8*rdo_ref.TABLE[(fmt, typ)][0], bits_after=8*rdo_ref.TABLE[(fmt, typ)][0])


@pytest.mark.parametrize("fmt,typ", ROWS, ids=IDS)
def test_sse_after_is_what_compare_measures(gpu_ctx, fmt, typ):
    img = synth.photo(4*(SEG + 3) - 1, 13, seed=fmt)
    plain = _encode(gpu_ctx, [img], fmt, typ)[0]
    mask = (True, True, True, fmt != rdo_ref.BC1_RGB)
    (out,), (st,) = gpu_ctx.rdo([plain], [img], fmt, typ, LAM, mask=mask)
    for payload, key in ((plain, "sse_before"), (out, "sse_after")):
        c = gpu_ctx.compare(payload, img, fmt, typ, mask=mask)
        assert st[key] == round(sum(c.sse[ch] for ch in c.compared())*255.0*255.0), key
        assert c.error_blocks == 0
    assert st["sse_after"] >= st["sse_before"] and st["blocks_changed"] > 0
    if fmt == rdo_ref.BC7:
        dec, errors = gpu_ctx.decode(out, fmt, typ, img.shape[1], img.shape[0])
        assert errors == 0
        # no block of the result is in the reserved mode, which decodes to zeros without being counted
        assert out.reshape(-1, 16)[:, 0].all()


def test_two_identical_calls_return_identical_bits(gpu_ctx):
    images = [synth.photo(4*(2*SEG + 5), 12, seed=5), synth.photo(40, 40, seed=6)]
    plain = _encode(gpu_ctx, images, Format.BC7, Type.UNorm)
    a = gpu_ctx.rdo(plain, images, Format.BC7, Type.UNorm, 3.0, max_sse_increase=500)
    b = gpu_ctx.rdo(plain, images, Format.BC7, Type.UNorm, 3.0, max_sse_increase=500)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]
    # lambda -> 0 changes almost nothing: only free improvements remain
    tiny, st = gpu_ctx.rdo(plain, images, Format.BC7, Type.UNorm, 0.01)
    assert all(s["sse_after"] <= s["sse_before"] for s in st)


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
    w, h, mips = 4*(SEG + 2) - 1, 20, 4
    plain, fused, source = (_texture(w, h, mips, dtype, int(fmt)) for _ in range(3))
    conv = {k: v for k, v in kw.items() if k != "max_sse_increase"}
    assert plain.convert(fmt, Type.UNorm, Quality.Low, **conv)
    assert fused.convert_rdo(fmt, Type.UNorm, Quality.Low, rdo_lambda=LAM, **kw)
    assert fused.converted() and (fused.format(), fused.type()) == (fmt, Type.UNorm)
    assert (fused.alpha_type(), fused.color_mask()) == (plain.alpha_type(), plain.color_mask())
    assert not fused.images_complete() and plain.rdo_stats() is None
    mask = list(kw.get("color_mask", (True,)*4))
    if kw.get("alpha_type") == Alpha.None_ or not Texture.has_alpha(fmt):
        mask[3] = False
    stats = fused.rdo_stats()
    assert len(stats) == mips
    for m in range(mips):
        src = source.get_image(m)
        src = src.astype(np.float32) if src.dtype == np.float16 else src          # convert() widens halves
        want, want_st = rdo_ref.rdo(plain.data(m), src, fmt, Type.UNorm, LAM, mask=mask,
                                    max_sse_increase=kw.get("max_sse_increase"))
        assert np.array_equal(fused.data(m), want), m
        assert stats[m] == want_st, m
    assert sum(s["blocks_changed"] for s in stats) > 0
