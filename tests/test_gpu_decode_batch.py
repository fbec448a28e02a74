"""Batched decode (cfhip_decode_batch*) on the GPU: bit-identical to the per-surface Context.decode, surface by
surface, with equal error-block counts; pixel-type outputs bit-identical to the numpy normalisation of
Texture.decode_image; the device form with odd pitches and unaligned pointers."""
import numpy as np
import pytest

from cuttlefish_amd import api
from test_gpu_decode import PAIRS, _bb, _foot, random_payload

pytestmark = pytest.mark.gpu

MIX = [(4096, 4096), (1, 1), (5, 3), (257, 130)]
DIV = {"RGBA8": 255.0, "R8": 255.0, "RG8": 255.0, "R8_SNorm": 127.0, "RG8_SNorm": 127.0, "R16": 2047.0,
       "RG16": 2047.0, "R16_SNorm": 1023.0, "RG16_SNorm": 1023.0}


def _nblocks(fmt, w, h):
    bw, bh = _foot(fmt)
    return ((w + bw - 1)//bw)*((h + bh - 1)//bh)


def _payloads(fmt, sizes, seed):
    return [random_payload(fmt, _nblocks(fmt, w, h), seed + i) for i, (w, h) in enumerate(sizes)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _normalised(raw, layout):
    """Texture.decode_image's numpy code"""
    h, w, n = raw.shape
    out = np.zeros((h, w, 4), np.float32)
    out[..., 3] = 1.0
    if layout == api.Layout.RGBA16F:
        val = raw.astype(np.float32)
    else:
        val = np.maximum(raw.astype(np.float64)/DIV[layout.name], -1.0).astype(np.float32)
    out[..., :n] = val
    return out


@pytest.mark.parametrize("fmt,typ", PAIRS)
def test_native_output_equals_decode_surface_by_surface(gpu_ctx, fmt, typ):
    pays = _payloads(fmt, MIX, fmt*16 + typ)
    outs, bad = gpu_ctx.decode_batch(pays, fmt, typ, MIX)
    total = 0
    for p, (w, h), got, b in zip(pays, MIX, outs, bad):
        want, want_bad = gpu_ctx.decode(p, fmt, typ, w, h)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(_bits(got), _bits(want)), (w, h)
        assert b == want_bad, (w, h, b, want_bad)
        total += b
    if fmt == 35 or fmt >= 43:
        assert total > 0 and len(set(bad)) > 1          # random blocks: errors occur, and differ per surface
    again, bad2 = gpu_ctx.decode_batch(pays, fmt, typ, MIX)
    assert bad2 == bad and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(outs, again))
    assert "decode_batch" in gpu_ctx.last_kernel_name()


@pytest.mark.parametrize("fmt,typ", [(29, 0), (33, 1), (35, 4), (36, 0), (40, 0), (42, 0), (43, 0), (47, 4), (56, 0)])
def test_a_300_surface_mip_tail_call(gpu_ctx, fmt, typ):
    sizes = [(1 + (i*7) % 37, 1 + (i*5) % 29) for i in range(300)]
    pays = _payloads(fmt, sizes, 9000 + fmt)
    outs, bad = gpu_ctx.decode_batch(pays, fmt, typ, sizes)
    for p, (w, h), got, b in zip(pays, sizes, outs, bad):
        want, want_bad = gpu_ctx.decode(p, fmt, typ, w, h)
        assert np.array_equal(_bits(got), _bits(want)) and b == want_bad, (w, h)


@pytest.mark.parametrize("fmt,typ", PAIRS)
def test_pixel_type_outputs_equal_the_numpy_normalisation(gpu_ctx, fmt, typ):
    sizes = [(257, 130), (5, 3), (64, 64)]
    pays = _payloads(fmt, sizes, 333 + fmt*8 + typ)
    layout, _ = api.decoded_layout(fmt, typ)
    native, bad = gpu_ctx.decode_batch(pays, fmt, typ, sizes)
    for pix in api.PixelType:
        cell = (pix == api.PixelType.RGBA32F or (pix == api.PixelType.RGBA8 and layout.name in ("RGBA8", "R8", "RG8")) or
                (pix == api.PixelType.RGBA16F and layout == api.Layout.RGBA16F))
        if not cell:
            with pytest.raises(api.CfhipError) as e:
                gpu_ctx.decode_batch(pays, fmt, typ, sizes, pix)
            assert e.value.code == api.E_UNSUPPORTED
            continue
        outs, bad2 = gpu_ctx.decode_batch(pays, fmt, typ, sizes, pix)
        assert bad2 == bad
        for raw, got in zip(native, outs):
            if pix == api.PixelType.RGBA32F:
                want = _normalised(raw, layout)
            elif pix == api.PixelType.RGBA16F:
                want = raw
            else:
                want = np.zeros(raw.shape[:2] + (4,), np.uint8)
                want[..., 3] = 255
                want[..., :raw.shape[2]] = raw
            assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), (pix, raw.shape)


@pytest.mark.parametrize("fmt,typ", [(29, 0), (33, 1), (34, 0), (35, 5), (36, 0), (41, 1), (44, 0), (55, 4)])
@pytest.mark.parametrize("pix", [None, api.PixelType.RGBA32F])
def test_device_form_with_odd_pitches_and_unaligned_pointers(gpu_ctx, fmt, typ, pix):
    import torch
    dev = torch.device("cuda", 0)
    sizes = [(133, 70), (9, 9), (64, 32), (31, 5)]
    pays = _payloads(fmt, sizes, 4242 + fmt)
    want, want_bad = gpu_ctx.decode_batch(pays, fmt, typ, sizes, pix)
    tb = want[0].shape[2]*want[0].dtype.itemsize
    # payloads packed with a 3-byte stagger, outputs with odd pitches at odd offsets (the first one aligned)
    blob = np.zeros(sum(p.nbytes + 3 for p in pays) + 16, np.uint8)
    boffs, o = [], 0
    for i, p in enumerate(pays):
        o += 0 if i == 0 else 3
        boffs.append(o)
        blob[o:o + p.nbytes] = p
        o += p.nbytes
    pitches = [w*tb + (64 if i == 0 else 3 + i) for i, (w, _) in enumerate(sizes)]
    ooffs, o = [], 0
    for i, ((w, h), pitch) in enumerate(zip(sizes, pitches)):
        o = (o + 255)//256*256 + (0 if i == 0 else i)
        ooffs.append(o)
        o += h*pitch
    d_blob = torch.from_numpy(blob).to(dev)
    d_out = torch.full((o + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_bad = torch.full((len(sizes),), -1, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu_ctx.decode_batch_device([dict(blocks=d_blob.data_ptr() + bo, out=d_out.data_ptr() + oo, width=w, height=h,
                                      out_pitch_bytes=pitch)
                                 for bo, oo, (w, h), pitch in zip(boffs, ooffs, sizes, pitches)],
                                fmt, typ, pix, error_blocks=d_bad.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    host = d_out.cpu().numpy()
    mask = np.zeros(host.size, bool)
    for oo, (w, h), pitch, arr in zip(ooffs, sizes, pitches, want):
        rows = host[oo:oo + h*pitch].reshape(h, pitch)
        assert np.array_equal(rows[:, :w*tb], _bits(arr).reshape(h, w*tb)), (w, h)
        m = mask[oo:oo + h*pitch].reshape(h, pitch)
        m[:, :w*tb] = True
    assert (host[~mask] == 0xAB).all()                      # nothing outside the surfaces is written
    assert [int(v) for v in d_bad.cpu()] == want_bad
