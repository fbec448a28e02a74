"""Who owns the stream codecs' stage times (the context's stage log, csrc/stage_log.h): after a call of one of the six
families -- estimator, deflate, inflate, LZ4 encode, LZ4 decode, PNG -- its own *_stage_ms answers with its stages and
the five others refuse; after a call that keeps no log all six refuse; while profiling the second of two calls still
answers; a device form given nothing to do owns the log and has no times."""
import numpy as np
import pytest

import lz4_cases as LC
from cuttlefish_amd import Format, Quality, Type, api, synth

pytestmark = pytest.mark.gpu

STAGE_MS = {"lz_size": ("lz_stage_ms", api.LZ_STAGES), "deflate": ("deflate_stage_ms", api.DEFLATE_STAGES),
            "inflate": ("inflate_stage_ms", api.INFLATE_STAGES), "lz4_encode": ("lz4_encode_stage_ms", api.LZ4_ENCODE_STAGES),
            "lz4_decode": ("lz4_decode_stage_ms", api.LZ4_DECODE_STAGES), "png_encode": ("png_stage_ms", api.PNG_STAGES)}
SLICE = 65536           # 70,000 bytes: two slices


def _owner_is(ctx, family, what):
    """only `family`'s *_stage_ms answers (None: none does)"""
    for name, (method, stages) in STAGE_MS.items():
        if name == family:
            ms = getattr(ctx, method)()
            assert tuple(ms) == stages and all(v >= 0.0 for v in ms.values()), (what, name, ms)
        else:
            with pytest.raises(api.CfhipError, match="the last call on this context was no"):
                getattr(ctx, method)()


@pytest.fixture
def two_slices(gpu_ctx):
    before = gpu_ctx.lz_slice_bytes(SLICE)
    yield gpu_ctx
    gpu_ctx.lz_slice_bytes(before if before != 4 << 20 else 0)


def test_each_family_owns_its_own_times(two_slices):
    ctx = two_slices
    a = LC.content("text", 70000)
    assert ctx.lz_size(a)["bytes_in"] == a.size
    _owner_is(ctx, "lz_size", "lz_size")
    z = ctx.deflate(a)
    _owner_is(ctx, "deflate", "deflate")
    zi, index = ctx.deflate_indexed(a)
    assert zi == z
    _owner_is(ctx, "deflate", "deflate_indexed")
    assert ctx.inflate(zi, index, a.size) == a.tobytes()
    _owner_is(ctx, "inflate", "inflate")
    frame = ctx.lz4_encode(a)
    _owner_is(ctx, "lz4_encode", "lz4_encode")
    assert ctx.lz4_decode(frame, a.size) == a.tobytes()
    _owner_is(ctx, "lz4_decode", "lz4_decode")
    image = (np.arange(5*3*4, dtype=np.uint32)*37 % 251).astype(np.uint8).reshape(3, 5, 4)
    assert ctx.png_encode(image)[:8] == b"\x89PNG\r\n\x1a\n"
    _owner_is(ctx, "png_encode", "png_encode")


def test_calls_that_own_no_log(gpu_ctx):
    a = LC.content("text", 4097)
    # a call of another part of the API: one BC1 block decoded
    gpu_ctx.deflate(a)
    gpu_ctx.decode(np.arange(8, dtype=np.uint8), Format.BC1_RGB, Type.UNorm, 4, 4)
    _owner_is(gpu_ctx, None, "decode")
    # the encoder's code builder alone: the encoder's kernel name, none of its stages
    gpu_ctx.deflate(a)
    gpu_ctx.deflate_code_lengths(np.arange(1, 20, dtype=np.uint32), 7)
    _owner_is(gpu_ctx, None, "deflate_code_lengths")
    # the target search runs the estimator several times and is no estimate
    img = synth.photo(100, 36, seed=int(Format.BC1_RGB))
    plain = gpu_ctx.encode([img], api.make_params(Format.BC1_RGB, Type.UNorm, Quality.Low))
    gpu_ctx.lz_size(a)
    gpu_ctx.rdo_target(plain, [img], Format.BC1_RGB, Type.UNorm, 0.9, 32.0)
    _owner_is(gpu_ctx, None, "rdo_target")


def test_second_call_while_profiling(gpu_ctx):
    a = LC.content("text", 4097)
    gpu_ctx.profile_begin()
    try:
        gpu_ctx.deflate(a)
        gpu_ctx.deflate(a)
        _owner_is(gpu_ctx, "deflate", "profiling")
    finally:
        gpu_ctx.profile_end()


def test_device_forms_with_nothing_to_do(gpu_ctx):
    import ctypes
    import torch
    a = LC.content("text", 4097)
    s = torch.cuda.Stream()
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(max(ctypes.sizeof(api.DeflateResult), ctypes.sizeof(api.Lz4Result)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.deflate(a)
    gpu_ctx.deflate_device([], out.data_ptr(), 64, res.data_ptr(), stream=s.cuda_stream)
    _owner_is(gpu_ctx, None, "deflate_device, empty")
    gpu_ctx.lz4_encode(a)
    gpu_ctx.lz4_encode_device([], out.data_ptr(), 64, res.data_ptr(), stream=s.cuda_stream)
    _owner_is(gpu_ctx, None, "lz4_encode_device, empty")
    s.synchronize()
