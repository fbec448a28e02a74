"""The zlib encoder on the GPU (csrc/deflate.hip) against its definition, tests/deflate_ref.py: the bytes equal, zlib
reading them back, every field of cfhip_deflate_result equal, through the host and the device form -- at the stream
lengths where the chunk, group and tail logic take another path, on contents that choose each form, use no distance
code, one literal, or exceed the 15-bit limit; in slices, in spans, the code builder alone, the argument errors, next to
the estimator on one context, and through Texture.pack."""
import ctypes
import zlib

import numpy as np
import pytest

import deflate_cases as C
import deflate_ref as D
import lzsize_ref as Z
from cuttlefish_amd import Format, Quality, Texture, Type, api, synth

pytestmark = pytest.mark.gpu

RESULT = ctypes.sizeof(api.DeflateResult)


def _device_form(ctx, spans, total, stream=0, fill=0xCD):
    """cfhip_deflate_device on (pointer, bytes) spans -> (the stream's bytes, the result dict)"""
    import torch
    cap = api.deflate_bound(total)
    out = torch.full((cap + 8,), fill, dtype=torch.uint8, device="cuda")
    res = torch.full((RESULT,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.deflate_device(spans, out.data_ptr(), cap, res.data_ptr(), stream=stream)
    if stream:
        torch.cuda.synchronize()
    r = api.DeflateResult.from_buffer_copy(res.cpu().numpy().tobytes()).as_dict()
    raw = out.cpu().numpy()
    assert (raw[cap:] == fill).all()                        # nothing is written past the bound
    return raw[:r["bytes_out"]].tobytes(), r


def _upload(a):
    import torch
    dev = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
    if a.size:
        dev[5:5 + a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()       # an unaligned span
    return dev, dev.data_ptr() + 5


@pytest.mark.parametrize("name,n", C.CASES, ids=C.IDS)
def test_bytes_are_the_twins(gpu_ctx, name, n):
    a = C.data(name, n)
    want, res = C.twin(name, n)
    got = gpu_ctx.deflate(a)
    assert got == want, (name, n, len(got), len(want))
    assert zlib.decompress(got) == a.tobytes()
    assert gpu_ctx.deflate_result() == res
    assert len(got) == res["bytes_out"] <= api.deflate_bound(n) == D.deflate_bound(n)
    keep, ptr = _upload(a)
    dev, dres = _device_form(gpu_ctx, [(ptr, n)] if n else [], n)
    assert dev == want and dres == res
    del keep


def test_slices_do_not_change_the_bytes(gpu_ctx):
    before = gpu_ctx.lz_slice_bytes(0)
    try:
        for name in ("text", "zeros", "no4gram", "random"):
            a = C.data(name, C.BIG)
            want, res = C.twin(name, C.BIG)
            gpu_ctx.lz_slice_bytes(0)
            whole = gpu_ctx.deflate(a)
            gpu_ctx.lz_slice_bytes(Z.COSTBLK)               # four slices, three of them behind a carried window
            sliced, sres = gpu_ctx.deflate(a), gpu_ctx.deflate_result()
            gpu_ctx.lz_slice_bytes(2*Z.COSTBLK)
            two = gpu_ctx.deflate(a)
            assert whole == sliced == two == want, name
            assert sres == res
    finally:
        gpu_ctx.lz_slice_bytes(before if before != 4 << 20 else 0)


def test_spans_are_their_concatenation(gpu_ctx):
    import torch
    a = np.concatenate([C.data("text", 70001), C.data("BC1", 32768)[:9999], C.data("zeros", 5000)])
    want, res = D.deflate(a)
    cuts = (0, 4097, 4097, 70001 + 33, a.size)
    assert gpu_ctx.deflate([a[s:e] for s, e in zip(cuts, cuts[1:])]) == want
    # the parts lie at odd offsets of one buffer, in another order than the stream's, around a zero-length span
    room = torch.zeros(2*a.size + 64, dtype=torch.uint8, device="cuda")
    place, spans = (1, 0, 100001, 4099 + 9), []
    for at, s, e in zip(place, cuts, cuts[1:]):
        if e > s:
            room[at:at + e - s] = torch.from_numpy(a[s:e]).cuda()
        spans.append((room.data_ptr() + at if e > s else 0, e - s))
    stream = torch.cuda.Stream()
    got, dres = _device_form(gpu_ctx, spans, a.size, stream=stream.cuda_stream)
    assert got == want and dres == res
    assert gpu_ctx.last_kernel_ms() > 0.0
    ms = gpu_ctx.deflate_stage_ms()
    assert tuple(ms) == api.DEFLATE_STAGES and all(v >= 0.0 for v in ms.values())
    single, _ = _device_form(gpu_ctx, [(room.data_ptr() + 1, 4097)], 4097)
    assert single == D.twin(a[:4097])


@pytest.mark.parametrize("name,counts,limit", C.HISTOGRAMS, ids=[h[0].replace(" ", "_") for h in C.HISTOGRAMS])
def test_code_builder_alone(gpu_ctx, name, counts, limit):
    want = D.code_lengths(counts, limit)
    got = gpu_ctx.deflate_code_lengths(counts, limit)
    assert got.tolist() == want.tolist(), name
    used = got[got > 0].astype(np.int64)
    assert int((1 << (limit - used)).sum()) <= 1 << limit and used.max() <= limit
    assert all(got[i] for i, c in enumerate(counts) if c)


def test_errors_leave_out_untouched(gpu_ctx):
    lib = api.load_library()
    a = C.data("text", 5000)
    cap = api.deflate_bound(a.size)
    out = np.full(cap, 0xEE, np.uint8)
    res = api.DeflateResult()
    span = (api.LzSpan*2)()
    span[0].bytes, span[0].n = a.ctypes.data, a.size

    def call(spans=span, n=1, out_ptr=out.ctypes.data, cap_=cap, res_ptr=ctypes.addressof(res)):
        return lib.cfhip_deflate(gpu_ctx._h, spans, n, out_ptr, cap_, res_ptr)
    assert call(cap_=cap - 1) == api.E_CAPACITY
    assert call(out_ptr=None) == api.E_INVALID
    assert call(spans=None, n=1) == api.E_INVALID
    span[1].bytes, span[1].n = None, 7
    assert call(n=2) == api.E_INVALID
    assert call(res_ptr=None) == api.E_INVALID
    assert (out == 0xEE).all()
    import torch
    dout = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    dres = torch.zeros(RESULT, dtype=torch.uint8, device="cuda")
    dev, ptr = _upload(a)
    torch.cuda.synchronize()
    for kw in (dict(cap=cap - 1), dict(out=0), dict(result=0), dict(out=dout.data_ptr() + 1)):
        args = dict(out=dout.data_ptr(), cap=cap, result=dres.data_ptr())
        args.update(kw)
        with pytest.raises(api.CfhipError):
            gpu_ctx.deflate_device([(ptr, a.size)], **args)
    with pytest.raises(api.CfhipError):
        gpu_ctx.deflate_device([(0, 9)], dout.data_ptr(), cap, dres.data_ptr())
    torch.cuda.synchronize()
    assert bool((dout == 0xEE).all())
    # and the good call still works afterwards
    assert call() == 0 and out[:res.bytes_out].tobytes() == D.twin(a)


def test_estimator_and_encoder_share_a_context(gpu_ctx):
    a = C.data("BC7", 65536)
    before = gpu_ctx.lz_size(a)
    stream = gpu_ctx.deflate(a)
    after = gpu_ctx.lz_size(a)
    assert before == after == Z.lz_size(a)
    res = gpu_ctx.deflate_result()
    assert [res[k] for k in ("literals", "matches", "matched_bytes")] == \
        [before[k] for k in ("literals", "matches", "matched_bytes")]
    assert stream == C.twin("BC7", 65536)[0]
    with pytest.raises(api.CfhipError):
        gpu_ctx.deflate_stage_ms()                          # the last call was an estimate


def test_texture_pack(gpu_ctx):
    mips = 7
    tex = Texture(64, 64, mip_levels=mips)
    assert tex.pack() is None and tex.pack_result() is None
    for m in range(mips):
        assert tex.set_image(synth.photo(tex.width(m), tex.height(m), seed=5 + m), m)
    assert tex.convert(Format.BC7, Type.UNorm, Quality.Low)
    packed = tex.pack()
    raw = b"".join(tex.data(m).tobytes() for m in range(mips))
    assert len(raw) > 4096 + 1024 and zlib.decompress(packed) == raw
    assert packed == D.twin(np.frombuffer(raw, np.uint8))
    res, est = tex.pack_result(), tex.packed_size()
    assert res["literals"] == est["literals"] and res["matches"] == est["matches"]
    assert res["bytes_in"] == len(raw) and res["bytes_out"] == len(packed)
