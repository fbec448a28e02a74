"""Indexed zlib streams on the GPU (csrc/inflate.hip) against their definition, tests/inflate_ref.py: the encoder's
index equal to build_index of its bytes, the inflated bytes and every field of cfhip_inflate_result equal to the twin's
through the host and the device form, an independent encoder's flushed streams, slices, the depth of the pointer
jumping, the verdict on every mutation with guard bytes around the output, the argument errors, spans, and a packed
texture unpacked and decoded without a host copy of its payload.

`rounds` is the depth of the longest copy chain inside one slice, so it is the one field that depends on the slice and
that the twin does not define: the slices test compares every other field (on zeros a slice of 65536 bytes holds a chain
of 65536, the unsliced 204800 bytes one of 204800)."""
import ctypes
import math

import numpy as np
import pytest

import deflate_cases as C
import deflate_ref as D
import inflate_cases as IC
import inflate_ref as I
import lzsize_ref as Z
from cuttlefish_amd import CubeFace, Dimension, Format, Quality, Texture, Type, api, synth

pytestmark = pytest.mark.gpu

RESULT = ctypes.sizeof(api.InflateResult)
GUARD = 256


def _no_rounds(res):
    return {k: v for k, v in res.items() if k != "rounds"}


def _device_inflate(ctx, z, index, n, stream=0):
    """cfhip_inflate_device on uploaded copies -> (the n bytes, the result dict); 0xAB guards on both sides of out"""
    import torch
    zd = torch.from_numpy(np.frombuffer(z, np.uint8).copy()).cuda() if len(z) else torch.zeros(4, dtype=torch.uint8, device="cuda")
    idx = IC.index_array(index)
    idd = torch.from_numpy(idx.view(np.int64).copy()).cuda() if idx.size else None
    room = torch.full((GUARD + n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    res = torch.full((RESULT,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.inflate_device(zd.data_ptr(), len(z), idd.data_ptr() if idd is not None else 0, idx.shape[0],
                       room.data_ptr() + GUARD if n else 0, n, res.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    raw = room.cpu().numpy()
    assert (raw[:GUARD] == 0xAB).all() and (raw[GUARD + n:] == 0xAB).all()       # nothing outside [out, out + n)
    r = api.InflateResult.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
    return raw[GUARD:GUARD + n].tobytes(), r


@pytest.mark.parametrize("name,n", C.CASES, ids=C.IDS)
def test_own_streams(gpu_ctx, name, n):
    a = C.data(name, n)
    want, dres = C.twin(name, n)
    stream, index = gpu_ctx.deflate_indexed(a)
    assert stream == want == gpu_ctx.deflate(a) and gpu_ctx.deflate_result() == dres
    assert index.shape == (api.zindex_entries(n), 2)
    assert [tuple(int(v) for v in e) for e in index] == IC.own_index(name, n)
    _, twin = IC.own_verdict(name, n)
    assert gpu_ctx.inflate(stream, index, n) == a.tobytes()
    res = gpu_ctx.inflate_result()
    assert _no_rounds(res) == twin and res["status"] == 0
    assert res["rounds"] <= (math.ceil(math.log2(n)) + 1 if n > 1 else 1)
    out, dev = _device_inflate(gpu_ctx, stream, index, n)
    assert out == a.tobytes() and dev == res


def test_deflate_indexed_device(gpu_ctx):
    import torch
    a = C.data("text", C.BIG)
    want, dres = C.twin("text", C.BIG)
    src = torch.from_numpy(a.copy()).cuda()
    cap, entries = api.deflate_bound(a.size), api.zindex_entries(a.size)
    out = torch.full((cap + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    idx = torch.full((entries + 1, 2), -1, dtype=torch.int64, device="cuda")
    res = torch.zeros(ctypes.sizeof(api.DeflateResult), dtype=torch.uint8, device="cuda")
    gpu_ctx.deflate_indexed_device([(src.data_ptr(), a.size)], out.data_ptr(), cap, idx.data_ptr(), entries,
                                   res.data_ptr())
    r = api.DeflateResult.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
    assert r == dres and out.cpu().numpy()[:r["bytes_out"]].tobytes() == want
    host = idx.cpu().numpy()
    assert [tuple(int(v) for v in e) for e in host[:entries]] == IC.own_index("text", C.BIG) and (host[entries] == -1).all()
    ms = gpu_ctx.deflate_stage_ms()
    assert tuple(ms) == api.DEFLATE_STAGES
    # straight into the inflater, nothing leaves the device
    back = torch.full((a.size,), 0xEE, dtype=torch.uint8, device="cuda")
    ires = torch.zeros(RESULT, dtype=torch.uint8, device="cuda")
    gpu_ctx.inflate_device(out.data_ptr(), r["bytes_out"], idx.data_ptr(), entries, back.data_ptr(), a.size, ires.data_ptr())
    assert api.InflateResult.from_buffer_copy(ires.cpu().numpy().tobytes()).status == 0
    assert bool((back == src).all())
    ms = gpu_ctx.inflate_stage_ms()
    assert tuple(ms) == api.INFLATE_STAGES and all(v >= 0.0 for v in ms.values()) and gpu_ctx.last_kernel_ms() > 0.0


@pytest.mark.parametrize("content,n,mode", IC.FOREIGN, ids=IC.FOREIGN_IDS)
def test_foreign_streams(gpu_ctx, content, n, mode):
    x, z, index = IC.foreign(content, n, mode)
    assert gpu_ctx.inflate(z, index, n) == x
    _, twin = IC.foreign_verdict(content, n, mode)
    assert _no_rounds(gpu_ctx.inflate_result()) == twin


def test_slices_do_not_change_the_result(gpu_ctx):
    before = gpu_ctx.lz_slice_bytes(0)
    try:
        for name in ("text", "zeros", "no4gram"):
            a = C.data(name, C.BIG)
            z, index = C.twin(name, C.BIG)[0], IC.own_index(name, C.BIG)
            gpu_ctx.lz_slice_bytes(0)
            whole, wres = gpu_ctx.inflate(z, index, C.BIG), gpu_ctx.inflate_result()
            gpu_ctx.lz_slice_bytes(Z.COSTBLK)               # four slices, pointers into the slices before
            sliced, sres = gpu_ctx.inflate(z, index, C.BIG), gpu_ctx.inflate_result()
            assert whole == sliced == a.tobytes(), name
            assert _no_rounds(wres) == _no_rounds(sres) and sres["rounds"] <= wres["rounds"], name
            dz, di = gpu_ctx.deflate_indexed(a)
            assert dz == z and [tuple(int(v) for v in e) for e in di] == index, name
    finally:
        gpu_ctx.lz_slice_bytes(before if before != 4 << 20 else 0)


def test_pointer_jumping_depth(gpu_ctx):
    """zeros: every byte copies the one before it, a chain no payload reaches"""
    n = C.BIG
    before = gpu_ctx.lz_slice_bytes(0)
    try:
        assert gpu_ctx.inflate(C.twin("zeros", n)[0], IC.own_index("zeros", n), n) == bytes(n)
        rounds = gpu_ctx.inflate_result()["rounds"]
        print("zeros-%d: rounds %d" % (n, rounds))
        assert 17 <= rounds <= math.ceil(math.log2(n)) + 1
    finally:
        gpu_ctx.lz_slice_bytes(before if before != 4 << 20 else 0)


def test_mutations(gpu_ctx):
    """error codes, not faults: (status, bad_chunk) of every mutation as the twin's (its verdicts as recorded in
    tests/golden/inflate_mutations.json, which tests/test_inflate_ref.py holds to the twin), the guards untouched"""
    muts, recorded = IC.mutations(), IC.recorded_verdicts()
    assert len(muts) == len(recorded) and all(m[0] == r[0] for m, r in zip(muts, recorded))
    for (label, z, index, n), (_, status, bad_chunk) in zip(muts, recorded):
        try:
            got = gpu_ctx.inflate(z, index, n)
            out, twin = I.inflate_indexed(z, index, n)          # the few that pass: the twin's bytes and result
            assert status == 0 and got == out and _no_rounds(gpu_ctx.inflate_result()) == twin, label
        except api.CfhipError as e:
            assert e.code == api.E_DATA and (e.status, e.bad_chunk) == (status, bad_chunk) and status, label
        res = gpu_ctx.inflate_result()
        assert (res["status"], res["bad_chunk"]) == (status, bad_chunk), (label, res)
        if status:
            assert res["bytes_out"] == 0 and res["adler32"] == 0, label
    # the device form with guards, on one mutation per class and original
    seen = set()
    for (label, z, index, n), (_, status, bad_chunk) in zip(muts, recorded):
        key = (label.split()[0], status)
        if key in seen:
            continue
        seen.add(key)
        _, dev = _device_inflate(gpu_ctx, z, index, n)
        assert (dev["status"], dev["bad_chunk"]) == (status, bad_chunk), (label, dev)
    assert {s for _, s in seen} >= set(range(1, 8))


def test_errors_leave_out_untouched(gpu_ctx):
    lib = api.load_library()
    a = C.data("text", 5000)
    z = np.frombuffer(D.twin(a), np.uint8).copy()
    index = IC.index_array(I.build_index(z.tobytes()))
    out = np.full(5000, 0xEE, np.uint8)
    res = api.InflateResult()

    def call(z_ptr=z.ctypes.data, zbytes=z.size, idx=index.ctypes.data, entries=2, out_ptr=out.ctypes.data, n=5000,
             res_ptr=ctypes.addressof(res)):
        return lib.cfhip_inflate(gpu_ctx._h, z_ptr, zbytes, idx, entries, out_ptr, n, res_ptr)
    assert call(entries=1) == api.E_CAPACITY
    assert call(z_ptr=None) == api.E_INVALID
    assert call(idx=None) == api.E_INVALID
    assert call(out_ptr=None) == api.E_INVALID
    assert call(res_ptr=None) == api.E_INVALID
    assert (out == 0xEE).all()
    import torch
    dout = torch.full((5000,), 0xEE, dtype=torch.uint8, device="cuda")
    dres = torch.zeros(RESULT, dtype=torch.uint8, device="cuda")
    dz = torch.from_numpy(z).cuda()
    di = torch.from_numpy(index.view(np.int64)).cuda()
    torch.cuda.synchronize()
    for kw in (dict(index_entries=1), dict(out=0), dict(result=0), dict(out=dout.data_ptr() + 1), dict(zstream=0),
               dict(index=di.data_ptr() + 4)):
        args = dict(zstream=dz.data_ptr(), zbytes=z.size, index=di.data_ptr(), index_entries=2, out=dout.data_ptr(),
                    out_bytes=5000, result=dres.data_ptr())
        args.update(kw)
        with pytest.raises(api.CfhipError):
            gpu_ctx.inflate_device(**args)
    torch.cuda.synchronize()
    assert bool((dout == 0xEE).all())
    # and the good call still works afterwards; the empty stream on the device form too
    assert call() == 0 and out.tobytes() == a.tobytes()
    _, r = _device_inflate(gpu_ctx, D.EMPTY, [], 0)
    assert r == dict(I.inflate_indexed(D.EMPTY, [], 0)[1], rounds=0)
    _, r = _device_inflate(gpu_ctx, D.EMPTY + b"\x00", [], 0)
    assert (r["status"], r["bad_chunk"]) == (I.E_WRAPPER, 0)


def test_estimator_encoder_and_inflater_share_a_context(gpu_ctx):
    a = C.data("BC7", 65536)
    before = gpu_ctx.lz_size(a)
    stream, index = gpu_ctx.deflate_indexed(a)
    assert gpu_ctx.inflate(stream, index, a.size) == a.tobytes()
    with pytest.raises(api.CfhipError):
        gpu_ctx.deflate_stage_ms()                          # the last call was an inflate
    assert gpu_ctx.lz_size(a) == before == Z.lz_size(a)
    with pytest.raises(api.CfhipError):
        gpu_ctx.inflate_stage_ms()                          # the last call was an estimate
    assert gpu_ctx.deflate(a) == stream == C.twin("BC7", 65536)[0]
    assert gpu_ctx.inflate(stream, index, a.size) == a.tobytes()


def test_spans_at_odd_offsets(gpu_ctx):
    import torch
    a = np.concatenate([C.data("text", 70001), C.data("BC1", 32768)[:9999], C.data("zeros", 5000)])
    want, res = D.deflate(a)
    cuts = (0, 4097, 4097, 70001 + 33, a.size)
    stream, index = gpu_ctx.deflate_indexed([a[s:e] for s, e in zip(cuts, cuts[1:])])
    assert stream == want and [tuple(int(v) for v in e) for e in index] == I.build_index(want)
    room = torch.zeros(2*a.size + 64, dtype=torch.uint8, device="cuda")
    place, spans = (1, 0, 100001, 4099 + 9), []
    for at, s, e in zip(place, cuts, cuts[1:]):
        if e > s:
            room[at:at + e - s] = torch.from_numpy(a[s:e]).cuda()
        spans.append((room.data_ptr() + at if e > s else 0, e - s))
    cap, entries = api.deflate_bound(a.size), api.zindex_entries(a.size)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    idx = torch.zeros((entries, 2), dtype=torch.int64, device="cuda")
    dres = torch.zeros(ctypes.sizeof(api.DeflateResult), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    gpu_ctx.deflate_indexed_device(spans, out.data_ptr(), cap, idx.data_ptr(), entries, dres.data_ptr(), stream=s.cuda_stream)
    # the inflate follows on the same stream, into an odd (4-byte aligned) place
    back = torch.full((a.size + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    ires = torch.zeros(RESULT, dtype=torch.uint8, device="cuda")
    gpu_ctx.inflate_device(out.data_ptr(), len(want), idx.data_ptr(), entries, back.data_ptr() + 4, a.size, ires.data_ptr(),
                           stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert api.DeflateResult.from_buffer_copy(dres.cpu().numpy().tobytes()).as_dict() == res
    r = api.InflateResult.from_buffer_copy(ires.cpu().numpy().tobytes()).as_dict()
    assert _no_rounds(r) == I.inflate_indexed(want, I.build_index(want), a.size)[1]
    host = back.cpu().numpy()
    assert host[4:4 + a.size].tobytes() == a.tobytes() and (host[:4] == 0xAB).all() and (host[4 + a.size:] == 0xAB).all()


def _textures():
    mips = 7
    tex = Texture(64, 64, mip_levels=mips)
    for m in range(mips):
        assert tex.set_image(synth.photo(tex.width(m), tex.height(m), seed=5 + m), m)
    assert tex.convert(Format.BC7, Type.UNorm, Quality.Low)
    cube = Texture(Dimension.Cube, 16, 16)
    for f in range(6):
        assert cube.set_image(synth.photo(16, 16, seed=20 + f), CubeFace(f))
    assert cube.convert(Format.BC1_RGB, Type.UNorm, Quality.Low)
    return (("BC7 mips", tex), ("BC1 cube", cube))


def test_texture_pack_unpack_decode(gpu_ctx):
    import torch
    for tag, tex in _textures():
        flat = tex._flat()
        raw = b"".join(p.tobytes() for _, _, _, p in flat)
        plain = tex.pack()
        stream, index = tex.pack(indexed=True)
        assert stream == plain == D.twin(np.frombuffer(raw, np.uint8)), tag
        assert tex.pack_result()["bytes_in"] == len(raw)
        back = Texture.unpack(tex, stream, index)
        assert back is not None and back.converted() and back.format() == tex.format() and back.type() == tex.type()
        assert (back.dimension(), back.width(), back.height(), back.mip_level_count(), back.face_count(),
                back.color_space(), back.alpha_type()) == \
            (tex.dimension(), tex.width(), tex.height(), tex.mip_level_count(), tex.face_count(), tex.color_space(),
             tex.alpha_type())
        for (m, d, f, p), (_, _, _, q) in zip(flat, back._flat()):
            assert np.array_equal(p, q), (tag, m, d, f)
        base = back._flat()[0][3].base
        assert all(q.base is base for _, _, _, q in back._flat())                 # one buffer, the surfaces views of it
        assert Texture.unpack(tex, stream[:-1], index) is None and Texture.unpack(tex, stream, index[:0]) is None
        # inflate_device -> decode_batch_device: the payload never visits the host
        ctx = tex._context()
        zd = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
        idd = torch.from_numpy(index.view(np.int64).copy()).cuda()
        payload = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
        ires = torch.zeros(RESULT, dtype=torch.uint8, device="cuda")
        ctx.inflate_device(zd.data_ptr(), len(stream), idd.data_ptr(), index.shape[0], payload.data_ptr(), len(raw),
                           ires.data_ptr())
        assert api.InflateResult.from_buffer_copy(ires.cpu().numpy().tobytes()).status == 0
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
            assert np.array_equal(o.cpu().numpy().view(np.uint32), want[m][d][f].view(np.uint32)), (tag, m, d, f)
