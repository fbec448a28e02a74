"""The deflate-size estimator on the GPU (csrc/lzsize.hip) against its definition, tests/lzsize_ref.py: every field of
cfhip_lz_stats equal, at the stream lengths where the kernels take another path (no key, one key, a chunk and a cost
block and their neighbours), at the edge of the window, for matches that overlap, hit the 258 cap or end at a chunk,
for the K-candidate rule, the lazy rule and ties, on random streams with and without matches, on real payloads as
one span and as three, through the device form on a caller's stream, and in slices with the carried window."""
import ctypes

import numpy as np
import pytest

import lzsize_ref as Z
from cuttlefish_amd import Format, Quality, Type, api, synth

pytestmark = pytest.mark.gpu


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)


def _letters(n, seed, k=4):
    return np.random.default_rng(seed).integers(0, k, n).astype(np.uint8)


def _same(ctx, spans, what=None):
    got, want = ctx.lz_size(spans), Z.lz_size(spans)
    assert got == want, (what, got, want)
    return want


def _place(n, seed, parts):
    """n bytes of noise with the byte strings of parts = {position: bytes} written over it"""
    a = _noise(n, seed)
    for at, b in parts.items():
        a[at:at + len(b)] = np.frombuffer(bytes(b), np.uint8)
    return a


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 4095, 4096, 4097, 65536 + 4096 + 17])
def test_lengths(gpu_ctx, n):
    want = _same(gpu_ctx, _letters(n, n), n)
    assert want["bytes_in"] == n and want["literals"] + want["matched_bytes"] == n
    if n > 4096:
        assert want["matches"] > n//20
    # one byte value throughout: one key, every match at distance 1
    _same(gpu_ctx, np.full(n, 0x5A, np.uint8), n)


def test_window_edge(gpu_ctx):
    pattern = bytes(_noise(64, 99))
    near = _place(Z.W + 4096, 1, {0: pattern, Z.W: pattern})                 # distance exactly W
    far = _place(Z.W + 4096, 1, {0: pattern, Z.W + 1: pattern})              # W + 1: outside
    a, b = _same(gpu_ctx, near, "W"), _same(gpu_ctx, far, "W + 1")
    assert a["matched_bytes"] >= 64 > b["matched_bytes"]
    L, D = Z.matches(near)
    assert (L[Z.W], D[Z.W]) == (64, Z.W)


def test_overlap_cap_and_chunk_end(gpu_ctx):
    run = _same(gpu_ctx, np.full(1000, 7, np.uint8), "run")
    # a literal, then 258 + 258 + 258 + 225 bytes at distance 1
    assert (run["literals"], run["matches"], run["matched_bytes"]) == (1, 4, 999)
    pattern = bytes(_noise(32, 5))
    cut6 = _place(2*Z.CHUNK, 2, {100: pattern, Z.CHUNK - 6: pattern})         # cut to 6 bytes by the chunk's end
    cut3 = _place(2*Z.CHUNK, 2, {100: pattern, Z.CHUNK - 3: pattern})         # cut to 3: no match
    a, b = _same(gpu_ctx, cut6, "cut to 6"), _same(gpu_ctx, cut3, "cut to 3")
    assert Z.matches(cut6)[0][Z.CHUNK - 6] == 6 and Z.matches(cut3)[0][Z.CHUNK - 3] == 3
    assert a["matched_bytes"] >= 6 and a["matched_bytes"] - b["matched_bytes"] >= 6 - 3


def test_candidates_lazy_and_ties(gpu_ctx):
    key = b"\x01\x02\x03\x04"
    long_ = key + bytes(range(200, 216))
    # the short ones share seven bytes with the long one, so the keys at the next three positions see the same five
    shorts = [long_[:7] + bytes([100 + i, 101 + i]) for i in range(4)]

    def stream(n_short):
        parts = {64: long_}
        for i in range(n_short):
            parts[512*(i + 1)] = shorts[i]
        parts[3000] = long_
        return _place(Z.CHUNK, 3, parts)
    five, four = stream(4), stream(3)         # the long one is the fifth / the fourth most recent occurrence
    assert Z.matches(five)[0][3000] == 7 and Z.matches(four)[0][3000] == len(long_)
    for what, a, length in (("fifth", five, 7), ("fourth", four, len(long_))):
        mp, ml, _ = Z.parse(a)[1]
        assert (3000, length) in zip(mp.tolist(), ml.tolist()), what
        _same(gpu_ctx, a, what)
    # lazy: "abcd" matches 4 at p, "bcdefghij" 9 at p + 1: a literal and the longer match
    lazy = _place(Z.CHUNK, 4, {50: b"abcdX", 700: b"bcdefghij", 2000: b"abcdefghij"})
    L, _ = Z.matches(lazy)
    assert (L[2000], L[2001]) == (4, 9)
    lits, (mp, ml, _) = Z.parse(lazy)
    assert 2000 in lits and (2001, 9) in zip(mp.tolist(), ml.tolist())
    _same(gpu_ctx, lazy, "lazy")
    # a tie: two sources of the same length, the nearer one's distance is coded
    tie = _place(Z.CHUNK, 6, {100: b"qrstuvw1", 3000: b"qrstuvw2", 3100: b"qrstuvw3"})
    L, D = Z.matches(tie)
    assert (L[3100], D[3100]) == (7, 100)
    want = _same(gpu_ctx, tie, "tie")
    other = tie.copy()
    other[3000:3008] = other[3008:3016]
    assert Z.lz_size(other)["bits_q16"] != want["bits_q16"]          # distance 3000 is priced otherwise


def test_random_streams(gpu_ctx):
    n = 3*Z.COSTBLK + 123
    a = _same(gpu_ctx, _letters(n, 11), "4 letters")
    b = _same(gpu_ctx, _noise(n, 12), "256 letters")
    assert a["matched_bytes"] > 0.9*n and b["matched_bytes"] < 100
    assert b["est_bytes"] > 0.99*n


@pytest.fixture(scope="module")
def payloads(gpu_ctx):
    """GPU-encoded payloads of synth.photo 256 x 256: plain, and after Context.rdo where the pass covers the format"""
    img = synth.photo(256, 256, seed=1)
    out = {}
    for fmt in (Format.BC1_RGB, Format.BC7, Format.ASTC_6x6, Format.ETC2_R8G8B8):
        p = gpu_ctx.encode([img], api.make_params(fmt, Type.UNorm, Quality.Low))[0]
        out[fmt.name] = p
        if api.rdo_supported(fmt, Type.UNorm):
            out[fmt.name + " rdo"] = gpu_ctx.rdo([p], [img], fmt, Type.UNorm, 8.0)[0][0]
    return out


def test_real_payloads_one_span_and_three(gpu_ctx, payloads):
    assert len(payloads) == 6
    for name, p in payloads.items():
        want = _same(gpu_ctx, p, name)
        cut = (p.size//3 + 1, 2*p.size//3 + 5)
        parts = [p[:cut[0]], p[cut[0]:cut[1]], np.zeros(0, np.uint8), p[cut[1]:]]
        assert gpu_ctx.lz_size(parts) == want, name
    for fmt in ("BC1_RGB", "BC7"):
        assert Z.lz_size(payloads[fmt + " rdo"])["est_bytes"] < Z.lz_size(payloads[fmt])["est_bytes"]
    # several payloads are one stream: matches reach across the seam
    both = [payloads["BC1_RGB"], payloads["BC1_RGB"]]         # 32768 bytes: the copy lies exactly W back
    want = _same(gpu_ctx, both, "twice")
    assert want["est_bytes"] < 1.5*Z.lz_size(both[0])["est_bytes"]


def test_device_form_and_identical_calls(gpu_ctx, payloads):
    import torch
    p = payloads["BC7 rdo"]
    want = Z.lz_size(p)
    size = ctypes.sizeof(api.LzStats)
    dev = torch.zeros(p.size + 8, dtype=torch.uint8, device="cuda")
    dev[3:3 + p.size] = torch.from_numpy(p).cuda()                    # an unaligned span
    out = torch.full((2*size,), 0xAB, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    cut = p.size//2 + 1
    spans = [(dev.data_ptr() + 3, cut), (dev.data_ptr() + 3 + cut, p.size - cut)]
    gpu_ctx.lz_size_device(spans, out.data_ptr(), stream=stream.cuda_stream)
    gpu_ctx.lz_size_device(spans, out.data_ptr() + size, stream=stream.cuda_stream)
    stream.synchronize()
    raw = out.cpu().numpy().tobytes()
    assert raw[:size] == raw[size:]
    assert api.LzStats.from_buffer_copy(raw[:size]).as_dict() == want
    assert gpu_ctx.last_kernel_ms() > 0.0
    ms = gpu_ctx.lz_stage_ms()
    assert set(ms) == set(api.LZ_STAGES) and all(v >= 0.0 for v in ms.values())
    # the context's stream, and an empty stream through the device form
    gpu_ctx.lz_size_device(spans[:1], out.data_ptr())
    assert api.LzStats.from_buffer_copy(out.cpu().numpy().tobytes()[:size]).as_dict() == Z.lz_size(p[:cut])
    gpu_ctx.lz_size_device([], out.data_ptr())
    assert not out.cpu().numpy()[:size].any()
    assert gpu_ctx.lz_size(p) == gpu_ctx.lz_size(p) == want


def test_slices_carry_the_window(gpu_ctx, payloads):
    # 200 KiB that match across every slice boundary: a payload repeated at a distance inside the window
    p = payloads["BC1_RGB"][:20000]
    a = np.concatenate([p]*11)[:200*1024]
    a[70000:70100] = _noise(100, 8)
    want = Z.lz_size(a)
    whole = gpu_ctx.lz_size(a)
    before = gpu_ctx.lz_slice_bytes(Z.COSTBLK)              # four slices, three of them behind a carried window
    try:
        assert gpu_ctx.lz_slice_bytes(Z.COSTBLK) == Z.COSTBLK
        sliced = gpu_ctx.lz_size(a)
        three = gpu_ctx.lz_size([a[:Z.COSTBLK - 7], a[Z.COSTBLK - 7:Z.COSTBLK + 9], a[Z.COSTBLK + 9:]])
        gpu_ctx.lz_slice_bytes(2*Z.COSTBLK + 1)             # rounded up to three cost blocks
        assert gpu_ctx.lz_slice_bytes(2*Z.COSTBLK + 1) == 3*Z.COSTBLK
        two = gpu_ctx.lz_size(a)
        # the slice is clamped to one cost block .. 2^30 before it is rounded: no size wraps to 0
        gpu_ctx.lz_slice_bytes(2**64 - 1)
        assert gpu_ctx.lz_slice_bytes(1) == 1 << 30
        assert gpu_ctx.lz_slice_bytes(Z.COSTBLK) == Z.COSTBLK
    finally:
        gpu_ctx.lz_slice_bytes(before if before != 4 << 20 else 0)
    assert whole == sliced == three == two == want
    assert want["matched_bytes"] > 0.9*a.size
