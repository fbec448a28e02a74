"""LZ4 frames on the GPU (csrc/lz4.hip) against their definition, tests/lz4_ref.py: the encoder's bytes and result
equal to the twin's through the host and the device form, spans, slices; the decoder on the twin's frames and on liblz4's
(tests/golden/lz4_foreign.npz -- the library itself is never loaded here), the two rejected kinds, the verdict on every
mutation with guard bytes around the output, and a packed texture unpacked and decoded without a host copy."""
import ctypes

import numpy as np
import pytest

import lz4_cases as LC
import lz4_ref as R
import lzsize_ref as Z
from cuttlefish_amd import Format, Quality, Texture, Type, api, synth

pytestmark = pytest.mark.gpu

RESULT = ctypes.sizeof(api.Lz4DecodeResult)
GUARD = 256


def _device_encode(ctx, spans_host, stream=0):
    """cfhip_lz4_encode_device on uploaded spans -> (the frame, the result dict); 0xAB behind the bound"""
    import torch
    total = sum(len(s) for s in spans_host)
    keep, spans = [], []
    for s in spans_host:
        t = torch.from_numpy(np.frombuffer(bytes(s), np.uint8).copy()).cuda() if len(s) else None
        keep.append(t)
        spans.append((t.data_ptr() if t is not None else 0, len(s)))
    cap = api.lz4_bound(total)
    out = torch.full((cap + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    res = torch.full((ctypes.sizeof(api.Lz4Result),), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.lz4_encode_device(spans, out.data_ptr(), cap, res.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    r = api.Lz4Result.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
    raw = out.cpu().numpy()
    assert (raw[cap:] == 0xAB).all()
    return raw[:r["bytes_out"]].tobytes(), r


def _device_decode(ctx, z, n, stream=0):
    """cfhip_lz4_decode_device on an uploaded copy -> (the n bytes, the result dict); 0xAB guards on both sides of out"""
    import torch
    zd = torch.from_numpy(np.frombuffer(z, np.uint8).copy()).cuda() if len(z) else torch.zeros(4, dtype=torch.uint8, device="cuda")
    room = torch.full((GUARD + n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    res = torch.full((RESULT,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.lz4_decode_device(zd.data_ptr(), len(z), room.data_ptr() + GUARD if n else 0, n, res.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    raw = room.cpu().numpy()
    assert (raw[:GUARD] == 0xAB).all() and (raw[GUARD + n:] == 0xAB).all()       # nothing outside [out, out + n)
    r = api.Lz4DecodeResult.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
    return raw[GUARD:GUARD + n].tobytes(), r


@pytest.mark.parametrize("name,n", LC.CASES, ids=LC.IDS)
def test_encode_and_decode_own_frames(gpu_ctx, name, n):
    a = LC.content(name, n)
    want, res = LC.twin(name, n)
    assert gpu_ctx.lz4_encode(a) == want and gpu_ctx.lz4_encode_result() == res
    frame, dres = _device_encode(gpu_ctx, [a.tobytes()])
    assert frame == want and dres == res
    back, twin = R.decode(want, n)
    assert back == a.tobytes()
    assert gpu_ctx.lz4_decode(want, n) == back and gpu_ctx.lz4_decode_result() == twin
    out, dev = _device_decode(gpu_ctx, want, n)
    assert out == back and dev == twin


def test_spans_against_their_concatenation(gpu_ctx):
    a = np.concatenate([LC.content("text", 70001), LC.content("BC1", 32768)[:9999], LC.content("zeros", 5000)])
    want, res = R.encode(a)
    cuts = (0, 4097, 4097, 70001 + 33, a.size)
    parts = [a[s:e] for s, e in zip(cuts, cuts[1:])]
    assert gpu_ctx.lz4_encode(parts) == want and gpu_ctx.lz4_encode_result() == res
    import torch
    s = torch.cuda.Stream()
    frame, dres = _device_encode(gpu_ctx, [p.tobytes() for p in parts], stream=s.cuda_stream)
    assert frame == want and dres == res
    out, dev = _device_decode(gpu_ctx, want, a.size, stream=s.cuda_stream)
    assert out == a.tobytes() and dev == R.decode(want, a.size)[1]


def test_slices_do_not_change_the_frame(gpu_ctx):
    before = gpu_ctx.lz_slice_bytes(0)
    try:
        for name in ("text", "zeros", "random"):
            a = LC.content(name, 200*1024)
            want, res = LC.twin(name, 200*1024)
            gpu_ctx.lz_slice_bytes(Z.COSTBLK)                   # four slices of one block
            assert gpu_ctx.lz4_encode(a) == want and gpu_ctx.lz4_encode_result() == res, name
            gpu_ctx.lz_slice_bytes(0)
            assert gpu_ctx.lz4_encode(a) == want and gpu_ctx.lz4_encode_result() == res, name
    finally:
        gpu_ctx.lz_slice_bytes(before if before != 4 << 20 else 0)


@pytest.mark.parametrize("which,i", LC.FOREIGN_ALL, ids=LC.FOREIGN_IDS)
def test_foreign_frames(gpu_ctx, which, i):
    x, z = LC.foreign(which, i)
    back, twin = R.decode(z, len(x))
    assert back == x and twin["content_checksum"] == (1 if which == "a" else 0)
    assert gpu_ctx.lz4_decode(z, len(x)) == x and gpu_ctx.lz4_decode_result() == twin
    out, dev = _device_decode(gpu_ctx, z, len(x))
    assert out == x and dev == twin


def test_rejected_frames_are_unsupported(gpu_ctx):
    for key in ("linked", "big"):
        z = LC.fixture()[key]
        twin = R.decode(z, 200*1024)[1]
        assert (twin["status"], twin["bad_block"]) == (R.E_UNSUPPORTED, 0)
        with pytest.raises(api.CfhipError) as e:
            gpu_ctx.lz4_decode(z, 200*1024)
        assert (e.value.code, e.value.status, e.value.bad_block) == (api.E_DATA, api.LZ4_UNSUPPORTED, 0)
        assert "unsupported" in str(e.value) and gpu_ctx.lz4_decode_result() == twin
        assert _device_decode(gpu_ctx, z, 200*1024)[1] == twin


def test_mutations(gpu_ctx):
    """classes, not faults: (status, bad_block) of every mutation as the twin's (its verdicts as recorded in
    tests/golden/lz4_mutations.json, which tests/test_lz4_ref.py holds to the twin); the device form, with guard bytes
    around out, on every record too"""
    muts, recorded = LC.mutations(), LC.recorded_verdicts()
    assert len(muts) == len(recorded) and all(m[0] == r[0] for m, r in zip(muts, recorded))
    seen = set()
    for (label, z, n), (_, status, bad_block) in zip(muts, recorded):
        try:
            got = gpu_ctx.lz4_decode(z, n)
            out, twin = R.decode(z, n)                          # the few that pass: the twin's bytes and result
            assert status == 0 and got == out and gpu_ctx.lz4_decode_result() == twin, label
        except api.CfhipError as e:
            assert e.code == api.E_DATA and (e.status, e.bad_block) == (status, bad_block) and status, label
        res = gpu_ctx.lz4_decode_result()
        assert (res["status"], res["bad_block"]) == (status, bad_block), (label, res)
        if status:
            assert res["bytes_out"] == 0 and res["sequences"] == 0, label
        _, dev = _device_decode(gpu_ctx, z, n)
        assert dev == res, (label, dev, res)
        seen.add(status)
    assert seen >= set(range(8))


def test_errors_and_stage_times(gpu_ctx):
    a = LC.content("text", 70000)
    frame = gpu_ctx.lz4_encode(a)
    ms = gpu_ctx.lz4_encode_stage_ms()
    assert tuple(ms) == api.LZ4_ENCODE_STAGES and all(v >= 0.0 for v in ms.values()) and gpu_ctx.last_kernel_ms() > 0.0
    with pytest.raises(api.CfhipError):
        gpu_ctx.lz4_decode_stage_ms()                       # the last call was an encode
    with pytest.raises(api.CfhipError):
        gpu_ctx.lz_stage_ms()
    with pytest.raises(api.CfhipError):
        gpu_ctx.deflate_stage_ms()
    assert gpu_ctx.lz4_decode(frame, a.size) == a.tobytes()
    ms = gpu_ctx.lz4_decode_stage_ms()
    assert tuple(ms) == api.LZ4_DECODE_STAGES and all(v >= 0.0 for v in ms.values())
    with pytest.raises(api.CfhipError):
        gpu_ctx.lz4_encode_stage_ms()
    # the estimator and the zlib encoder share the scratch and are not disturbed
    assert gpu_ctx.lz_size(a) == Z.lz_size(a)
    import zlib
    assert zlib.decompress(gpu_ctx.deflate(a)) == a.tobytes()
    assert gpu_ctx.lz4_encode(a) == frame
    # the empty frame on the device forms
    f, r = _device_encode(gpu_ctx, [])
    assert f == R.EMPTY and r == R.encode(b"")[1]
    _, r = _device_decode(gpu_ctx, R.EMPTY, 0)
    assert r == R.decode(R.EMPTY, 0)[1]
    _, r = _device_decode(gpu_ctx, R.EMPTY + b"\x00", 0)
    assert (r["status"], r["bad_block"]) == (R.E_BLOCKS, 0)
    import torch
    dout = torch.full((70000,), 0xEE, dtype=torch.uint8, device="cuda")
    dres = torch.zeros(RESULT, dtype=torch.uint8, device="cuda")
    dz = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    for kw in (dict(out=0), dict(result=0), dict(out=dout.data_ptr() + 1), dict(frame=0), dict(result=dres.data_ptr() + 4)):
        args = dict(frame=dz.data_ptr(), nbytes=len(frame), out=dout.data_ptr(), out_bytes=70000, result=dres.data_ptr())
        args.update(kw)
        with pytest.raises(api.CfhipError):
            gpu_ctx.lz4_decode_device(**args)
    torch.cuda.synchronize()
    assert bool((dout == 0xEE).all())


def test_texture_pack_lz4_unpack_decode(gpu_ctx):
    import torch
    mips = 7
    tex = Texture(64, 64, mip_levels=mips)
    for m in range(mips):
        assert tex.set_image(synth.photo(tex.width(m), tex.height(m), seed=5 + m), m)
    assert tex.convert(Format.BC7, Type.UNorm, Quality.Low)
    flat = tex._flat()
    raw = b"".join(p.tobytes() for _, _, _, p in flat)
    frame = tex.pack(codec="lz4")
    assert frame == R.twin(np.frombuffer(raw, np.uint8)) and frame[:4] == api.LZ4_MAGIC
    assert tex.pack_result()["bytes_in"] == len(raw) and tex.pack_result()["bytes_out"] == len(frame)
    with pytest.raises(ValueError):
        tex.pack(indexed=True, codec="lz4")
    back = Texture.unpack(tex, frame)
    assert back is not None and back.converted() and back.format() == tex.format() and back.type() == tex.type()
    assert (back.width(), back.height(), back.mip_level_count()) == (tex.width(), tex.height(), tex.mip_level_count())
    for (m, d, f, p), (_, _, _, q) in zip(flat, back._flat()):
        assert np.array_equal(p, q), (m, d, f)
    assert Texture.unpack(tex, frame[:-1]) is None
    # the zlib path is as it was
    stream, index = tex.pack(indexed=True)
    assert Texture.unpack(tex, stream, index) is not None and tex.pack() == stream
    # lz4_decode_device -> decode_batch_device: the payload never visits the host
    ctx = tex._context()
    zd = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).cuda()
    payload = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    dres = torch.zeros(RESULT, dtype=torch.uint8, device="cuda")
    ctx.lz4_decode_device(zd.data_ptr(), len(frame), payload.data_ptr(), len(raw), dres.data_ptr())
    assert api.Lz4DecodeResult.from_buffer_copy(dres.cpu().numpy().tobytes()).status == 0
    want = tex.decode_images()
    surfaces, outs, at = [], [], 0
    for m, d, f, p in flat:
        w, h = tex.width(m), tex.height(m)
        o = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        outs.append(o)
        surfaces.append(dict(blocks=payload.data_ptr() + at, blocks_bytes=p.nbytes, width=w, height=h,
                             out=o.data_ptr(), out_pitch_bytes=w*16))
        at += p.nbytes
    ctx.decode_batch_device(surfaces, tex.format(), tex.type(), api.PixelType.RGBA32F)
    torch.cuda.synchronize()
    for (m, d, f, _), o in zip(flat, outs):
        assert np.array_equal(o.cpu().numpy().view(np.uint32), want[m][d][f].view(np.uint32)), (m, d, f)
