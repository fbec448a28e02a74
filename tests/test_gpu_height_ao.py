"""Ambient occlusion from height maps on the GPU (cfhip_height_ao_array_device) against its numpy twin
(tests/height_ao_ref.py, fed the library's direction table), byte for byte: the channels of the mask, the channels left
alone, the gaps of the pitches, the sources and the records."""
import os
import re

import numpy as np
import pytest

import height_ao_ref as R
from cuttlefish_amd import ColorSpace, CubeFace, Dimension, Image, ResizeFilter, Texture, api, process_image

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = (np.uint8, np.float16, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SHARED = open(os.path.join(ROOT, "cuttlefish_amd", "csrc", "height_ao.h")).read()
TILE_W = int(re.search(r"CFHAO_TILE_W = (\d+);", _SHARED).group(1))
TILE_H = int(re.search(r"CFHAO_TILE_H = (\d+);", _SHARED).group(1))                  # up to R = 16
TILE_H_WIDE = int(re.search(r"CFHAO_TILE_H_WIDE = (\d+);", _SHARED).group(1))        # above
_TABLES = {}


def table(D):
    if D not in _TABLES:
        _TABLES[D] = api.height_ao_directions(D)
    return _TABLES[D]


def heights(h, w, dtype, seed=0):
    """(h, w, 4) smooth bumps plus noise in every channel, each channel another field"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([0.5 + 0.25*np.sin(x*(0.3 + 0.1*c) + seed) * np.cos(y*(0.2 + 0.07*c)) + 0.2*rng.random((h, w))
                    for c in range(4)], -1)
    if dtype == np.uint8:
        return np.round(np.clip(img, 0, 1)*255).astype(np.uint8)
    return img.astype(dtype)


def noise(shape, dtype, seed):
    """a destination before the call: random bytes, NaN patterns among them"""
    rng = np.random.default_rng(700 + seed)
    return rng.integers(0, 256, shape + (4*np.dtype(dtype).itemsize,), dtype=np.uint8).view(dtype)


def upload(img, pad):
    """the image on the device with `pad` texels of 0xEE bytes after each row -> (byte tensor, pitch in bytes)"""
    h, w = img.shape[:2]
    row = w*4*img.itemsize
    buf = np.full((h, row + pad*4*img.itemsize), 0xEE, np.uint8)
    buf[:, :row] = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
    return torch.from_numpy(buf).cuda(), buf.shape[1]


def download(t, like):
    """-> (the image of `like`'s shape and dtype, whether the gap after the rows is still 0xEE)"""
    h, w = like.shape[:2]
    row = w*4*like.itemsize
    b = t.cpu().numpy()
    return np.ascontiguousarray(b[:, :row]).view(like.dtype).reshape(h, w, 4), bool((b[:, row:] == 0xEE).all())


def run(ctx, srcs, dst_dtype, radius, pad=0, dpad=0, in_place=False, records=True, stream=0, **kw):
    """one call on uploaded copies -> (the destinations before it, after it, the records as dicts or None)"""
    h, w = srcs[0].shape[:2]
    n = len(srcs)
    dsrc = [upload(im, pad) for im in srcs]
    before = list(srcs) if in_place else [noise((h, w), dst_dtype, 13*l + w) for l in range(n)]
    ddst = dsrc if in_place else [upload(b, dpad) for b in before]
    res = torch.full((n + 1, 4), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                               # the context's stream does not wait for torch's
    ctx.height_ao_device([t.data_ptr() for t, _ in dsrc], api.pixel_type_of(srcs[0]), w, h, dsrc[0][1],
                         [t.data_ptr() for t, _ in ddst], api.pixel_type_of(before[0]), ddst[0][1], radius=radius,
                         results=res.data_ptr() if records else 0, stream=stream, **kw)
    if stream:
        torch.cuda.synchronize()
    after = []
    for (t, _), b in zip(ddst, before):
        img, gap = download(t, b)
        assert gap, "the gap after a destination's rows was written"
        after.append(img)
    if not in_place:
        for (t, _), im in zip(dsrc, srcs):
            img, gap = download(t, im)
            assert gap and img.tobytes() == np.ascontiguousarray(im).tobytes(), "a source was written"
    rec = res.cpu().numpy()
    if not records:
        assert (rec == -1).all()
        return before, after, None
    assert (rec[-1] == -1).all(), "a record past the layers was written"
    rec = rec[:-1].copy().view(api.HEIGHT_AO_RESULT_DTYPE).reshape(n)
    return before, after, [{f: int(rec[l][f]) for f in R.FIELDS} for l in range(n)]


def check(ctx, srcs, dst_dtype, radius, D=16, channel=0, mask=1, height=1.0, strength=1.0, bias=0.0, uniform=False,
          falloff=False, wrap=(False, False), **kw):
    """the call against the twin, layer by layer -> the records"""
    before, after, rec = run(ctx, srcs, dst_dtype, radius, height_scale=height, directions=D, channel=channel,
                             channels=mask, strength=strength, bias=bias, uniform=uniform, falloff=falloff, wrap=wrap, **kw)
    flags = (R.WRAP_X if wrap[0] else 0) | (R.WRAP_Y if wrap[1] else 0) | (R.UNIFORM if uniform else 0) | \
        (R.FALLOFF if falloff else 0)
    for l, (src, b, a) in enumerate(zip(srcs, before, after)):
        want, wrec = R.height_ao(src, b, radius, height, D, channel, mask, strength, bias, flags, table(D))
        diff = (a.view(np.uint8) != want.view(np.uint8)).reshape(a.shape[0], a.shape[1], -1).any(-1)
        assert a.tobytes() == want.tobytes(), (l, int(diff.sum()), np.argwhere(diff)[:4].tolist(), a[diff][:2], want[diff][:2])
        if rec is not None:
            assert rec[l] == wrec, l
    return rec


SIZES = [(1, 1), (2, 1), (5, 3)] + [(TILE_W + dx, rows + dy) for rows in (TILE_H, TILE_H_WIDE)
                                    for dx, dy in ((-1, -1), (0, 0), (1, 1), (-1, 1), (1, -1))]


@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_around_the_tile(gpu_ctx, w, h):
    """the smallest surfaces, one narrower than every radius, and one below, at and above both tiles on each axis, at a
    radius of every halo class"""
    for radius, D in ((1, 8), (7, 16), (20, 32), (40, 8)):
        check(gpu_ctx, [heights(h, w, np.float32, seed=w + h)], np.float32, radius, D=D, height=6.0)
    check(gpu_ctx, [heights(h, w, np.uint8, seed=w)], np.uint8, 9, height=40.0, wrap=(True, True))
    assert gpu_ctx.last_kernel_ms() >= 0.0


def test_a_halo_wider_than_the_tile_over_several_tiles(gpu_ctx):
    w, h = 129, 37
    for wrap in ((False, False), (True, True)):
        rec = check(gpu_ctx, [heights(h, w, np.float32, seed=3)], np.float32, 64, D=32, height=12.0, wrap=wrap)
        assert 0 < rec[0]["occluded"] <= w*h


@pytest.mark.parametrize("D", (8, 16, 32))
@pytest.mark.parametrize("radius", (1, 2, 3, 16, 17, 32, 33, 64))
def test_directions_and_radii(gpu_ctx, D, radius):
    """every direction set at the radii where a family gains its first sample and on both sides of every halo class"""
    w, h = 70, 21
    check(gpu_ctx, [heights(h, w, np.float16, seed=D + radius)], np.float32, radius, D=D, height=8.0, bias=0.01)


@pytest.mark.parametrize("wrap", [(False, False), (True, False), (False, True), (True, True)])
def test_wrap(gpu_ctx, wrap):
    """3 x 5 at R = 7 is walked several times over; 70 x 40 wraps across tiles"""
    check(gpu_ctx, [heights(5, 3, np.float32, seed=5)], np.float32, 7, D=32, height=3.0, wrap=wrap)
    check(gpu_ctx, [heights(5, 3, np.uint8, seed=6)], np.float16, 7, D=8, height=30.0, wrap=wrap, falloff=True)
    check(gpu_ctx, [heights(40, 70, np.float32, seed=7)], np.float32, 24, D=16, height=5.0, wrap=wrap)


@pytest.mark.parametrize("sdtype", DTYPES)
@pytest.mark.parametrize("ddtype", DTYPES)
def test_pixel_types(gpu_ctx, sdtype, ddtype):
    """3 x 3 source and destination types; the 8-bit store rounds floor(v * 255 + 0.5), the half one to nearest-even"""
    w, h = 33, 19
    check(gpu_ctx, [heights(h, w, sdtype, seed=8)], ddtype, 6, D=16, height=25.0, mask=5)
    check(gpu_ctx, [heights(h, w, sdtype, seed=9)], ddtype, 3, D=8, height=4.0, mask=2, uniform=True)


@pytest.mark.parametrize("channel", [0, 1, 2, 3])
def test_each_channel(gpu_ctx, channel):
    w, h = 21, 9
    a = check(gpu_ctx, [heights(h, w, np.float32, seed=10)], np.float32, 5, channel=channel, height=7.0)
    check(gpu_ctx, [heights(h, w, np.uint8, seed=10)], np.uint8, 5, channel=channel, height=30.0)
    check(gpu_ctx, [heights(h, w, np.float16, seed=10)], np.float16, 5, channel=channel, height=7.0)
    assert a[0]["occluded"] > 0


@pytest.mark.parametrize("mask", [1, 8, 5, 15])
def test_masks(gpu_ctx, mask):
    w, h = 21, 9
    for dtype in DTYPES:
        check(gpu_ctx, [heights(h, w, np.float32, seed=11)], dtype, 4, mask=mask, height=9.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_with_the_mask_on_the_height_channel(gpu_ctx, dtype):
    """all heights are read before anything is written: several tiles, a halo that crosses them"""
    w, h = 150, 40
    scale = 60.0 if dtype == np.uint8 else 9.0
    for channel, mask in ((0, 1), (2, 15), (1, 2 | 8)):
        check(gpu_ctx, [heights(h, w, dtype, seed=12 + s) for s in range(2)], dtype, 20, channel=channel, mask=mask,
              height=scale, in_place=True, pad=3)


def test_pitches_with_a_gap(gpu_ctx):
    w, h = 33, 17
    for sdtype, ddtype, pad, dpad in ((np.uint8, np.float32, 5, 1), (np.float16, np.uint8, 1, 7), (np.float32, np.float16, 2, 3)):
        check(gpu_ctx, [heights(h, w, sdtype, seed=13)], ddtype, 6, height=20.0, pad=pad, dpad=dpad)


def test_special_heights(gpu_ctx):
    """NaN and the infinities read 0, denormals and signed zeros are heights like any other"""
    w, h = 40, 20
    img = heights(h, w, np.float32, seed=14)
    rng = np.random.default_rng(15)
    flat = img[..., 0].reshape(-1)
    for value in (np.nan, np.inf, -np.inf, 1e-40, -1e-42, -0.0, 3e38, -3e38):
        flat[rng.integers(0, flat.size, 12)] = value
    img[..., 0] = flat.reshape(h, w)
    for uniform in (False, True):
        check(gpu_ctx, [img], np.float32, 6, D=32, height=1.0, uniform=uniform)
        check(gpu_ctx, [img], np.float32, 6, D=16, height=3e38, uniform=uniform)       # products up to 1e77
        check(gpu_ctx, [img], np.float32, 6, D=8, height=1e-30, uniform=uniform)
    half = heights(h, w, np.float16, seed=16)
    hf = half[..., 1].reshape(-1)
    for value in (np.nan, np.inf, -np.inf, 6e-8, -6e-8, 65504.0):
        hf[rng.integers(0, hf.size, 12)] = value
    half[..., 1] = hf.reshape(h, w)
    check(gpu_ctx, [half], np.float16, 5, channel=1, height=2.0)
    tiny = np.zeros((h, w, 4), np.float32)
    tiny[..., 0] = rng.integers(0, 5, (h, w))*np.float32(1e-45)                       # denormal steps
    check(gpu_ctx, [tiny], np.float32, 4, height=1.0)
    check(gpu_ctx, [tiny], np.float32, 4, height=3e38)


def test_staircases_and_flat_surfaces(gpu_ctx):
    w, h = 70, 18
    stairs = np.zeros((h, w, 4), np.uint8)
    stairs[..., 0] = (np.arange(w)//5*17 % 256)[None, :]
    stairs[..., 3] = (np.arange(h)//3*40 % 256)[:, None]
    for channel in (0, 3):
        rec = check(gpu_ctx, [stairs], np.uint8, 8, channel=channel, height=10.0)
        assert rec[0]["occluded"] > 0
    for dtype in DTYPES:
        flat = np.full((h, w, 4), 77 if dtype == np.uint8 else 0.3, dtype)
        for D in (8, 16, 32):
            _, after, rec = run(gpu_ctx, [flat], dtype, 9, directions=D, height_scale=50.0, strength=2.5, wrap=(True, False))
            one = 255 if dtype == np.uint8 else 1.0
            assert (after[0][..., 0] == one).all()
            assert rec[0] == dict(occluded=0, darkest=0x3F800000, reserved0=0, reserved1=0)


@pytest.mark.parametrize("strength", [0.0, 1.0, 2.5])
def test_strength_bias_and_negative_height(gpu_ctx, strength):
    w, h = 45, 23
    img = [heights(h, w, np.float32, seed=17)]
    rec = check(gpu_ctx, img, np.float32, 7, height=12.0, strength=strength)
    check(gpu_ctx, img, np.uint8, 7, height=-12.0, strength=strength, bias=0.25)
    check(gpu_ctx, img, np.float16, 7, height=12.0, strength=strength, bias=0.5, uniform=True, falloff=True)
    if strength == 0.0:
        assert rec[0]["darkest"] == 0x3F800000 and rec[0]["occluded"] > 0
    if strength == 2.5:
        assert rec[0]["darkest"] == 0                       # clamped at 0
    none = check(gpu_ctx, img, np.float32, 7, height=12.0, strength=strength, bias=1e4)
    assert none[0] == dict(occluded=0, darkest=0x3F800000, reserved0=0, reserved1=0)


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("falloff", [False, True])
def test_both_visibilities_and_the_falloff(gpu_ctx, uniform, falloff):
    w, h = 45, 23
    for D, radius in ((8, 5), (16, 16), (32, 40)):
        check(gpu_ctx, [heights(h, w, np.float32, seed=18)], np.float32, radius, D=D, height=10.0, uniform=uniform,
              falloff=falloff, wrap=(False, True))


def test_three_layers_of_different_content_and_no_records(gpu_ctx):
    w, h = 65, 31
    imgs = [heights(h, w, np.uint8, seed=20 + s) for s in range(2)] + [np.full((h, w, 4), 9, np.uint8)]
    rec = check(gpu_ctx, imgs, np.float32, 10, height=30.0)
    assert rec[0] != rec[1] and rec[2] == dict(occluded=0, darkest=0x3F800000, reserved0=0, reserved1=0)
    assert check(gpu_ctx, imgs, np.uint8, 10, height=30.0, records=False) is None


def test_identical_calls_return_identical_bytes_and_the_time_answers(gpu_ctx):
    w, h = 130, 70
    imgs = [heights(h, w, np.float32, seed=s) for s in (22, 23)]
    kw = dict(directions=32, height_scale=9.0, channels=3)
    a = run(gpu_ctx, imgs, np.float32, 33, **kw)
    ms = gpu_ctx.last_kernel_ms()
    assert ms > 0.0 and gpu_ctx.last_kernel_name() == "cfhip_height_ao_scan_kernel"
    b = run(gpu_ctx, imgs, np.float32, 33, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2] == b[2]


def test_entry_frame_row(gpu_ctx):
    """in the manner of test_gpu_entry_frame: the name the call leaves, its two event pairs inside and outside a
    profile, and the context's own stream against a stream of the caller's"""
    imgs = [heights(8, 8, np.uint8, seed=s) for s in (24, 25)]
    kw = dict(directions=8, height_scale=20.0)
    gpu_ctx.profile_begin()
    try:
        a = run(gpu_ctx, imgs, np.uint8, 2, **kw)
        name, ms = gpu_ctx.last_kernel_name(), gpu_ctx.last_kernel_ms()
    finally:
        total, n = gpu_ctx.profile_end()
    assert name == "cfhip_height_ao_scan_kernel" and n == 2 and ms >= 0.0 and total >= 0.0
    b = run(gpu_ctx, imgs, np.uint8, 2, **kw)
    assert gpu_ctx.last_kernel_name() == name and gpu_ctx.last_kernel_ms() >= 0.0
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = run(gpu_ctx, imgs, np.uint8, 2, stream=s.cuda_stream, **kw)
    assert gpu_ctx.last_kernel_ms() >= 0.0
    for other in (b, c):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1], other[1])) and a[2] == other[2]
    # a refused call enqueues nothing and leaves the name alone
    with pytest.raises(api.CfhipError, match="height_ao: params->radius 65 outside 1 to 64"):
        p = api.make_height_ao_params(64)
        p.radius = 65
        t = torch.zeros(8*8*4, dtype=torch.uint8, device="cuda")
        gpu_ctx._check(gpu_ctx._lib.cfhip_height_ao_array_device(
            gpu_ctx._h, api._ptr_array([t.data_ptr()]), 1, 0, 8, 8, 32, api._ptr_array([t.data_ptr()]), 0, 32, p, None, None))
    assert gpu_ctx.last_kernel_name() == name


def test_host_conveniences(gpu_ctx):
    w, h = 37, 22
    img = heights(h, w, np.uint8, seed=26)
    out, rec = gpu_ctx.height_ao(img, 6, 25.0, 32, "g", "ra", 1.5, 0.05, True, True, (True, False))
    flags = R.WRAP_X | R.UNIFORM | R.FALLOFF
    want, wrec = R.height_ao(img, img, 6, 25.0, 32, 1, 9, 1.5, 0.05, flags, table(32))
    assert out.dtype == np.uint8 and out.tobytes() == want.tobytes() and rec == wrec
    out, rec = gpu_ctx.height_ao(img, 6, 25.0, out_dtype=np.float32)
    want, wrec = R.height_ao(img, np.zeros((h, w, 4), np.float32), 6, 25.0, table=table(16))
    assert out.dtype == np.float32 and out.tobytes() == want.tobytes() and rec == wrec
    im = Image(img, ColorSpace.Linear)
    ao = im.ambient_occlusion(6, 25.0, directions=8, channel="b", channels="g", wrap=True)
    want, _ = R.height_ao(img, img, 6, 25.0, 8, 2, 2, flags=R.WRAP_X | R.WRAP_Y, table=table(8))
    assert isinstance(ao, Image) and ao.pixels.dtype == np.uint8 and ao.pixels.tobytes() == want.tobytes()
    assert im.pixels.tobytes() == img.tobytes()             # a new image
    assert ao.save_bytes() == Image(want, ColorSpace.Linear).save_bytes()
    assert Image(np.ones((4, 4, 4), np.float32), rgbf=True).ambient_occlusion(2) is None


@pytest.mark.parametrize("dim,depth", [(Dimension.Cube, 0), (Dimension.Dim2D, 3)])
def test_texture_equals_the_context_path(gpu_ctx, dim, depth):
    w, h = 48, 48
    faces = list(CubeFace) if dim == Dimension.Cube else [None]
    hts, orm = Texture(dim, w, h, depth, 1), Texture(dim, w, h, depth, 1)
    src, dst = {}, {}
    for d in range(max(depth, 1)):
        for f in faces:
            args = (0, d) if f is None else (f, 0, d)
            s = 30 + 10*d + (int(f) if f is not None else 0)
            src[(d, f)] = heights(h, w, np.float32 if s % 2 else np.uint8, seed=s)
            dst[(d, f)] = heights(h, w, np.uint8, seed=100 + s)
            assert hts.set_image(src[(d, f)], *args) and orm.set_image(dst[(d, f)], *args)
    get = lambda t, f, d: t.get_image(0, d) if f is None else t.get_image(f, 0, d)      # noqa: E731
    assert orm.ao_results() == []
    kw = dict(radius=9, height=15.0, directions=32, strength=1.5, wrap=(True, False))
    assert orm.height_ambient_occlusion(hts, channel="g", height_channel="b", **kw) is True
    records = orm.ao_results()
    assert len(records) == max(depth, 1)*len(faces)
    assert [(r["mip"], r["depth"], r["face"]) for r in records] == sorted((r["mip"], r["depth"], r["face"]) for r in records)
    for d in range(max(depth, 1)):
        for fi, f in enumerate(faces):
            _, after, rec = run(gpu_ctx, [src[(d, f)]], np.uint8, 9, height_scale=15.0, directions=32, channel=2, channels=2,
                                strength=1.5, wrap=(True, False))
            want = dst[(d, f)].copy()
            want[..., 1] = after[0][..., 1]
            got = get(orm, f, d)
            assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), (d, f)
            assert get(hts, f, d).tobytes() == src[(d, f)].tobytes()
            mine = [r for r in records if (r["mip"], r["depth"], r["face"]) == (0, d, fi)][0]
            assert mine["occluded"] == rec[0]["occluded"]
            assert np.float32(mine["darkest"]).view(np.uint32) == rec[0]["darkest"]
    # the texture may hold its own heights: the height channel itself is overwritten
    d, f = max(depth, 1) - 1, faces[-1]
    assert hts.height_ambient_occlusion(hts, channel="b", height_channel="b", radius=9, height=15.0) is True
    _, after, _ = run(gpu_ctx, [src[(d, f)]], src[(d, f)].dtype, 9, height_scale=15.0, channel=2, channels=4, in_place=True)
    assert get(hts, f, d).tobytes() == after[0].tobytes()
    # the intended order: occlusion on level 0, then the chain
    assert orm.generate_mipmaps(ResizeFilter.Box) and orm.mip_level_count() == 6


def test_process_image_occludes_between_the_ops_and_the_resize(gpu_ctx):
    img = heights(20, 24, np.uint8, seed=60)
    kw = dict(filter=ResizeFilter.Box)
    ops_only = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 24, 20, **kw)         # the colour-space pass alone
    assert ops_only.shape == (20, 24, 4) and ops_only.dtype == np.float32
    ao = dict(radius=5, height=20.0, directions=32, channel="g", channels="b", strength=1.2, bias=0.02, uniform=True,
              falloff=True, wrap=(False, True))
    occluded, rec = R.height_ao(ops_only, ops_only, 5, 20.0, 32, 1, 4, 1.2, 0.02, R.WRAP_Y | R.UNIFORM | R.FALLOFF, table(32))
    assert rec["occluded"] > 0
    want = process_image(occluded, ColorSpace.Linear, ColorSpace.Linear, 12, 10, **kw)      # the resize alone
    got = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 10, ao=ao, **kw)
    plain = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 10, **kw)
    assert got.shape == (10, 12, 4) and got.tobytes() == want.tobytes() and got.tobytes() != plain.tobytes()
    assert process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 10, ao=None, **kw).tobytes() == plain.tobytes()
    # nothing resized: after the one ops pass
    same = process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 24, 20, ao=ao)
    assert same.tobytes() == occluded.tobytes()
    with pytest.raises(ValueError):
        process_image(img, ColorSpace.sRGB, ColorSpace.Linear, 12, 10, normal_map=(0, 1.0), ao=ao)
