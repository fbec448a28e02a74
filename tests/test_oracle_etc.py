"""ETC1 / ETC2 / EAC oracle: self-consistency (no independent ETC decoder exists in this
environment -- parity for this family is decoder-self-consistent only),
reference boundary semantics and structural known answers from the public specification."""
import numpy as np
import pytest

import oracle_lib as O
from cuttlefish_amd import synth
from etc_cases import etc_mode as _etc_mode

ETC1, RGB, A1, A8, R11, RG11 = 37, 38, 39, 40, 41, 42


@pytest.mark.parametrize("fmt,bs", [(ETC1, 8), (RGB, 8), (A1, 8), (A8, 16), (R11, 8), (RG11, 16)])
def test_reference_black_image_size_contract(fmt, bs):
    """lib/test/TextureTest.cpp:824-845"""
    img = np.zeros((16, 16, 4), np.float32)
    img[..., 3] = 1.0
    blk = O.encode(img, fmt)
    assert blk.nbytes == 16 * bs
    if fmt <= A8:
        dec = O.decode_etc(blk, fmt, 16, 16)
        assert (dec[..., :3] == 0).all() and (dec[..., 3] == 255).all()
    else:
        assert (O.decode_eac(blk, fmt, 16, 16) <= 4).all()


def test_known_answer_individual_block_from_spec_layout():
    """Hand-built ETC1 individual block: base colours 0xF/0x0 grey, tables 0, all selectors
    'large positive' (msb 0, lsb 1) -> left half 255 (clamped), right half 0+8."""
    blk = np.array([0xF0, 0xF0, 0xF0, 0x00, 0x00, 0x00, 0xFF, 0xFF], np.uint8)
    dec = O.decode_etc(blk, ETC1, 4, 4)
    assert (dec[:, :2, :3] == 255).all() and (dec[:, 2:, :3] == 8).all()
    blk[3] = 0x01                                   # flip bit: top / bottom halves
    dec = O.decode_etc(blk, ETC1, 4, 4)
    assert (dec[:2, :, :3] == 255).all() and (dec[2:, :, :3] == 8).all()


def test_known_answer_eac_block():
    """EAC alpha: base 100, multiplier 2, table 13 {-1,-2,-3,-10,0,1,2,9}: selector 4 -> 100,
    selector 7 -> 118, selector 3 -> 80."""
    sel = [4] * 16
    sel[0], sel[15] = 7, 3                          # column-major texel 0 and 15
    bits = 0
    for k, s in enumerate(sel):
        bits |= s << (45 - 3 * k)
    blk = np.array([100, (2 << 4) | 13] + [(bits >> (40 - 8 * i)) & 255 for i in range(6)], np.uint8)
    rgb = np.zeros(8, np.uint8)
    dec = O.decode_etc(np.concatenate([blk, rgb]), A8, 4, 4)
    a = dec[..., 3]
    assert a[0, 0] == 118 and a[3, 3] == 80 and a[1, 1] == 100


def test_quality_ladder_and_planar_gain():
    img = synth.photo(128, 128, seed=1, alpha=False)
    p1 = synth.psnr(img, O.decode_etc(O.encode(img, ETC1, quality=2, threads=4), ETC1, 128, 128), slice(0, 3))
    p2 = synth.psnr(img, O.decode_etc(O.encode(img, RGB, quality=2, threads=4), RGB, 128, 128), slice(0, 3))
    p4 = synth.psnr(img, O.decode_etc(O.encode(img, RGB, quality=4, threads=4), RGB, 128, 128), slice(0, 3))
    assert p1 > 35.0 and p2 >= p1 and p4 >= p2 - 1e-9
    # a planar ramp is (nearly) exact in ETC2 and poor in ETC1
    g = np.zeros((4, 4, 4), np.uint8)
    g[..., 3] = 255
    for y in range(4):
        for x in range(4):
            g[y, x, :3] = (x * 60, y * 60, 128)
    e2 = np.abs(O.decode_etc(O.encode(g, RGB), RGB, 4, 4)[..., :3].astype(int) - g[..., :3]).max()
    e1 = np.abs(O.decode_etc(O.encode(g, ETC1), ETC1, 4, 4)[..., :3].astype(int) - g[..., :3]).max()
    assert e2 <= 3 and e1 > 20


def test_a1_punch_through_and_a8_alpha():
    img = synth.photo(64, 64, seed=4, alpha=True)
    dec = O.decode_etc(O.encode(img, A1, quality=2, threads=4), A1, 64, 64)
    tr = img[..., 3] < 128
    assert tr.any() and (~tr).any()
    assert (dec[..., 3][tr] == 0).all() and (dec[..., 3][~tr] == 255).all()
    d = (dec[..., :3].astype(float) - img[..., :3])[~tr]
    assert 10 * np.log10(255 ** 2 / np.mean(d * d)) > 33.0
    dec8 = O.decode_etc(O.encode(img, A8, quality=2, threads=4), A8, 64, 64)
    assert synth.psnr(img, dec8, slice(3, 4)) > 45.0


@pytest.mark.parametrize("typ", [0, 1])
def test_r11_rg11_quantisation(typ):
    """unsigned: round(clamp(f,0,1)*2047); signed: round(clamp(f,-1,1)*1023)."""
    yy, xx = np.mgrid[0:32, 0:32]
    f = np.zeros((32, 32, 4), np.float32)
    f[..., 0] = xx / 31.0 if typ == 0 else (xx - 15.5) / 12.0
    f[..., 1] = np.sin(yy / 5.0) * 0.9 if typ else (np.sin(yy / 5.0) * 0.45 + 0.5)
    for fmt, nch in ((R11, 1), (RG11, 2)):
        dec = O.decode_eac(O.encode(f, fmt, typ=typ, quality=2), fmt, 32, 32, typ)
        lo, scale = (-1, 1023) if typ else (0, 2047)
        want = np.round(np.clip(f[..., :nch], lo, 1) * scale)
        assert np.abs(dec - want).max() <= (40 if typ == 0 else 24)


def test_partial_blocks_ignore_out_of_image_texels():
    """EtcConverter::process hands only the in-image region to the codec (:122-129): what
    lies outside must not influence the block."""
    img = synth.photo(6, 6, seed=3)
    a = np.pad(img, ((0, 2), (0, 2), (0, 0)), mode="edge")
    blk = O.encode(img, RGB, quality=1).reshape(-1, 8)
    full = O.encode(a, RGB, quality=1).reshape(-1, 8)
    assert np.array_equal(blk[0], full[0])           # interior block identical
    # ignoring the out-of-image texels can only help the in-image ones
    dec = O.decode_etc(blk.reshape(-1), RGB, 6, 6)
    dec_full = O.decode_etc(full.reshape(-1), RGB, 8, 8)[:6, :6]
    assert synth.psnr(img, dec, slice(0, 3)) >= synth.psnr(img, dec_full, slice(0, 3)) - 0.5


def test_threads_deterministic():
    img = synth.photo(64, 64, seed=2)
    assert np.array_equal(O.encode(img, A8, threads=1), O.encode(img, A8, threads=4))


def test_two_colour_blocks_use_t_or_h_mode_and_etc1_never_does():
    rng = np.random.default_rng(12)
    img = np.zeros((16, 16, 4), np.uint8)
    img[..., 3] = 255
    cols = [((200, 40, 30), (20, 60, 220)), ((250, 250, 10), (10, 120, 10)),
            ((128, 0, 128), (0, 160, 160)), ((255, 255, 255), (180, 20, 20))]
    k = 0
    for by in range(0, 16, 4):
        for bx in range(0, 16, 4):
            a, b = cols[k % 4]
            k += 1
            m = rng.random((4, 4)) < 0.45                      # scattered two-colour pattern
            blk = np.where(m[..., None], np.array(a), np.array(b)).astype(np.int16)
            blk += rng.integers(-3, 4, blk.shape)
            img[by:by + 4, bx:bx + 4, :3] = np.clip(blk, 0, 255)
    out2 = O.encode(img, 38, quality=2)                        # ETC2 RGB
    modes = [_etc_mode(out2[i:i + 8]) for i in range(0, out2.size, 8)]
    assert sum(m in (1, 2) for m in modes) >= 12, modes         # chroma edges need two base colours
    dec2 = O.decode_etc(out2, 38, 16, 16)
    out1 = O.encode(img, 37, quality=2)                        # ETC1: no ETC2 modes available
    assert all(_etc_mode(out1[i:i + 8]) == 0 for i in range(0, out1.size, 8))
    dec1 = O.decode_etc(out1, 37, 16, 16)
    e2 = np.mean((dec2[..., :3].astype(float) - img[..., :3])**2)
    e1 = np.mean((dec1[..., :3].astype(float) - img[..., :3])**2)
    assert e2 < 40 and e2 < e1/4, (e1, e2)


def test_hand_built_t_and_h_blocks_decode_to_their_paint_colours():
    # T: A = (15,0,0) -> 255,0,0; B = (0,0,15); distance index 3 (16); selectors 0,1,2,3 in column 0
    def be(hi, lo):
        return np.frombuffer(hi.to_bytes(4, "big") + lo.to_bytes(4, "big"), np.uint8)
    r1a, r1b = 3, 3
    hi = (7 << 29) | (r1a << 27) | (r1b << 24) | (0 << 20) | (0 << 16) | (0 << 12) | (0 << 8) | (15 << 4) | \
        ((3 >> 1) << 2) | (1 << 1) | (3 & 1)
    sel = [0, 1, 2, 3]                                         # texels (x=0, y=0..3): k = y
    lo = sum(((s >> 1) << (16 + k)) | ((s & 1) << k) for k, s in enumerate(sel))
    px = O.decode_etc(be(hi, lo), 38, 4, 4)
    assert px[0, 0, :3].tolist() == [255, 0, 0]
    assert px[1, 0, :3].tolist() == [16, 16, 255]              # B + 16, clamped
    assert px[2, 0, :3].tolist() == [0, 0, 255]
    assert px[3, 0, :3].tolist() == [0, 0, 239]                # B - 16, clamped at 0
    # H: c1 = (8,8,8) = 136, c2 = (2,2,2) = 34, w1 >= w2 -> low bit of the index set: da=0, db=1 -> index 3 (16)
    r1, g1, b1, r2, g2, b2 = 8, 8, 8, 2, 2, 2
    g1a, g1b, b1a, b1b = g1 >> 1, g1 & 1, b1 >> 3, b1 & 7
    hi = (1 << 31 if g1a >= 4 else 0) | (r1 << 27) | (g1a << 24) | (g1b << 20) | (b1a << 19) | (b1b << 15) | \
        (r2 << 11) | (g2 << 7) | (b2 << 3) | (0 << 2) | (1 << 1) | 1
    a, b = (g1b << 1) | b1a, b1b >> 1
    hi |= (7 << 21) if a + b >= 4 else (1 << 18)
    px = O.decode_etc(be(hi, lo), 38, 4, 4)
    assert _etc_mode(be(hi, lo)) == 2
    assert [px[y, 0, 0] for y in range(4)] == [136 + 16, 136 - 16, 34 + 16, 34 - 16]


def test_th_modes_in_punch_through_blocks():
    """RGB8A1 blocks with transparent texels may use the T / H modes too (paint colour 2 is the
    transparent one): the alpha mask must survive exactly and the opaque texels gain quality."""
    rng = np.random.default_rng(0)
    img = synth.photo(128, 128, seed=3).copy()
    img[..., 3] = np.where(rng.random((128, 128)) < 0.2, 0, 255)
    opaque = img[..., 3] == 255
    psnr = {}
    for q in (0, 1, 2):
        enc = O.encode(img, A1, quality=q, threads=4)
        dec = O.decode_etc(enc, A1, 128, 128)
        assert np.array_equal(dec[..., 3] == 255, opaque)
        d = (dec[..., :3].astype(np.float64) - img[..., :3].astype(np.float64))[opaque]
        psnr[q] = 10*np.log10(255.0**2/np.mean(d*d))
        if q >= 1:
            # the T / H encodings are in use: opaque flag clear (bit 33) with an R or G overflow
            hi = enc.reshape(-1, 8)[:, :4].astype(np.uint32)
            w = (hi[:, 0] << 24) | (hi[:, 1] << 16) | (hi[:, 2] << 8) | hi[:, 3]
            r = (w >> 27) & 31
            dr = ((w >> 24) & 7).astype(np.int64)
            dr = np.where(dr >= 4, dr - 8, dr)
            punch = ((w >> 1) & 1) == 0
            assert np.any(punch & ((r.astype(np.int64) + dr < 0) | (r.astype(np.int64) + dr > 31)))
    assert psnr[1] > psnr[0] + 2.0 and psnr[2] >= psnr[1]
