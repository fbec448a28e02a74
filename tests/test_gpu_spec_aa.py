"""Specular anti-aliasing on the GPU (cfhip_spec_aa_array_device) against its numpy twin (tests/spec_aa_ref.py), bit for
bit: the rewritten channel of every level as uint32, the three channels left alone, the sources and the records."""
import numpy as np
import pytest

import spec_aa_ref as R
from cuttlefish_amd import CubeFace, Dimension, ResizeFilter, Texture, api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = (np.uint8, np.float16, np.float32)
SIZES = [(2, 2), (3, 3), (5, 3), (7, 5), (33, 17), (63, 63), (64, 64), (65, 31), (95, 40), (130, 70), (1, 64), (64, 1),
         (2048, 2)]
# bit patterns no arithmetic would leave behind, NaN payloads among them
SENTINELS = np.array([0x7FC12345, 0xFFFFFFFF, 0x7F800001, 0xFFC00000, 0x80000000, 0x00000001, 0x7F7FFFFF, 0xDEADBEEF],
                     np.uint32)


def normal_map(h, w, dtype, signed=False, seed=0, strength=0.7):
    """(h, w, 4) bumpy normals in the unorm or the signed storage; alpha is noise"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.normal(0, strength, (h, w, 2)), np.ones((h, w, 1))], -1)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    img = np.concatenate([v if signed else v*0.5 + 0.5, rng.random((h, w, 1))], -1)
    if dtype == np.uint8:
        return np.round(np.clip(img, 0, 1)*255).astype(np.uint8)
    return img.astype(dtype)


def rough_map(h, w, dtype, seed=0):
    """(h, w, 4) random roughness in every channel; the float types carry sentinels, out-of-range values and NaN too"""
    rng = np.random.default_rng(500 + seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    img = (rng.random((h, w, 4))*1.3 - 0.1).astype(dtype)
    flat = img.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size//16))] = np.nan
    flat[rng.integers(0, flat.size, max(1, flat.size//16))] = np.inf
    return img


def level_shapes(w, h, count):
    return [(max(1, h >> k), max(1, w >> k)) for k in range(1, count)]


def prefill(shape, seed):
    """a level before the call: sentinel bit patterns in every channel"""
    rng = np.random.default_rng(900 + seed)
    return SENTINELS[rng.integers(0, len(SENTINELS), shape + (4,))]


def upload(img, pad):
    """the image on the device with `pad` texels of 0xEE bytes after each row -> (byte tensor, pitch in bytes)"""
    h, w = img.shape[:2]
    row = w*4*img.itemsize
    buf = np.full((h, row + pad*4*img.itemsize), 0xEE, np.uint8)
    buf[:, :row] = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
    return torch.from_numpy(buf).cuda(), buf.shape[1]


def unchanged(t, img):
    h, w = img.shape[:2]
    row = w*4*img.itemsize
    b = t.cpu().numpy()
    return b[:, :row].tobytes() == np.ascontiguousarray(img).tobytes() and (b[:, row:] == 0xEE).all()


def run(ctx, normals, rough, count, channel=1, pad=0, rpad=0, same=False, stream=0, **kw):
    """one call on uploaded copies -> (the levels before it [layer][k], after it, the records [layer][k] as dicts).
    rough: a list of images, or a float (no map).  same: the roughness is read from the normals' own surfaces."""
    h, w = normals[0].shape[:2]
    n = len(normals)
    nsrc = [upload(im, pad) for im in normals]
    maps = isinstance(rough, list)
    rsrc = nsrc if same else ([upload(im, rpad) for im in rough] if maps else None)
    before = [[prefill(s, 31*l + k) for k, s in enumerate(level_shapes(w, h, count))] for l in range(n)]
    dev = [[torch.from_numpy(b.view(np.int32)).cuda() for b in layer] for layer in before]
    per = count - 1
    res = torch.full((n*per + 1, 4), -1, dtype=torch.int32, device="cuda")
    if maps or same:
        kw.update(rough0=[t.data_ptr() for t, _ in rsrc], rough_pixel_type=api.pixel_type_of(normals[0] if same else rough[0]),
                  rough_pitch=rsrc[0][1])
    else:
        kw.update(base_roughness=rough)
    ctx.specular_aa_device([t.data_ptr() for t, _ in nsrc], api.pixel_type_of(normals[0]), w, h, nsrc[0][1],
                           [[t.data_ptr() for t in layer] for layer in dev], channel=channel, results=res.data_ptr(),
                           stream=stream, **kw)
    if stream:
        torch.cuda.synchronize()
    after = [[t.cpu().numpy().view(np.uint32) for t in layer] for layer in dev]
    for (t, _), im in zip(nsrc, normals):
        assert unchanged(t, im), "the normal map was written"
    if maps and not same:
        for (t, _), im in zip(rsrc, rough):
            assert unchanged(t, im), "level 0 of the roughness was written"
    rec = res.cpu().numpy()
    assert (rec[-1] == -1).all(), "a record past the levels was written"
    rec = rec[:-1].copy().view(api.SPEC_AA_RESULT_DTYPE).reshape(n, per)
    return before, after, [[{f: int(rec[l][k][f]) for f in R.FIELDS} for k in range(per)] for l in range(n)]


def check(ctx, normals, rough, count, channel=1, perceptual=True, signed_normals=False, reconstruct_z=False,
          variance_scale=1.0, max_variance=1.0, same=False, **kw):
    """the call against the twin, layer by layer and level by level -> the records"""
    before, after, rec = run(ctx, normals, rough, count, channel, same=same, perceptual=perceptual,
                             signed_normals=signed_normals, reconstruct_z=reconstruct_z, variance_scale=variance_scale,
                             max_variance=max_variance, **kw)
    flags = (R.PERCEPTUAL if perceptual else 0) | (R.SIGNED_NORMALS if signed_normals else 0) | \
        (R.RECONSTRUCT_Z if reconstruct_z else 0)
    for l, nm in enumerate(normals):
        r0 = nm if same else (rough[l] if isinstance(rough, list) else rough)
        values, wrec = R.specular_aa(nm, r0, count, channel, flags, variance_scale, max_variance)
        for k, (b, a, v) in enumerate(zip(before[l], after[l], values)):
            want = b.copy()
            want[..., channel] = v.view(np.uint32)
            assert a.shape == want.shape and a.dtype == np.uint32
            assert a.tobytes() == want.tobytes(), (l, k + 1, int((a != want).any(-1).sum()), a[a != want][:4], want[a != want][:4])
            assert rec[l][k] == wrec[k], (l, k + 1)
    return rec


@pytest.mark.parametrize("w,h", SIZES)
def test_every_size_full_chain(gpu_ctx, w, h):
    """the smallest surfaces, odd ends that make 3 x 3 footprints, one tile, a tile and one, a last tile wider than a
    tile (95), several tiles each way, a single column and row, and 12 levels: every launch of the chain"""
    count = R.chain_levels(w, h)
    n = [normal_map(h, w, np.uint8, seed=w + h)]
    check(gpu_ctx, n, [rough_map(h, w, np.float32, seed=w)], count)
    check(gpu_ctx, [normal_map(h, w, np.float32, signed=True, seed=w)], 0.5, count, signed_normals=True, perceptual=False)
    assert gpu_ctx.last_kernel_ms() >= 0.0


def test_partial_chains(gpu_ctx):
    """3 of 7 levels, and counts on both sides of a launch's five levels"""
    w, h = 95, 40
    n, r = [normal_map(h, w, np.float16, seed=1)], [rough_map(h, w, np.uint8, seed=2)]
    assert R.chain_levels(w, h) == 7
    for count in (2, 3, 5, 6, 7):
        check(gpu_ctx, n, r, count)
    check(gpu_ctx, [normal_map(2, 2048, np.uint8, seed=3)], 0.3, 11)      # two launches, the second one full


def test_three_layers_of_different_content(gpu_ctx):
    w, h = 65, 31
    n = [normal_map(h, w, np.uint8, seed=s, strength=0.2*(s + 1)) for s in range(3)]
    r = [rough_map(h, w, np.float16, seed=s) for s in range(3)]
    rec = check(gpu_ctx, n, r, R.chain_levels(w, h), channel=2)
    assert rec[0] != rec[1] != rec[2]
    check(gpu_ctx, [normal_map(2, 2048, np.float32, seed=s) for s in range(3)], 0.25, 12)


@pytest.mark.parametrize("ndtype", DTYPES)
@pytest.mark.parametrize("rdtype", DTYPES)
def test_pixel_types_mixed(gpu_ctx, ndtype, rdtype):
    w, h = 33, 17
    check(gpu_ctx, [normal_map(h, w, ndtype, seed=5)], [rough_map(h, w, rdtype, seed=6)], 6, channel=0)
    check(gpu_ctx, [normal_map(h, w, ndtype, seed=7)], 0.4, 6, channel=3)


@pytest.mark.parametrize("signed,recz", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("perceptual", [False, True])
def test_normal_storages_and_both_encodings(gpu_ctx, signed, recz, perceptual):
    w, h = 63, 63
    for dtype in (np.uint8, np.float32):
        if signed and dtype == np.uint8:
            continue                                   # 8 bits hold no sign
        n = normal_map(h, w, dtype, signed=signed, seed=11)
        if recz:
            n[..., 2] = 255 if dtype == np.uint8 else np.float32(-7.0)     # the stored blue is ignored
        check(gpu_ctx, [n], [rough_map(h, w, np.uint8, seed=12)], 6, signed_normals=signed, reconstruct_z=recz,
              perceptual=perceptual)


@pytest.mark.parametrize("channel", [0, 1, 2, 3])
def test_each_channel(gpu_ctx, channel):
    w, h = 7, 5
    check(gpu_ctx, [normal_map(h, w, np.float32, seed=13)], [rough_map(h, w, np.float32, seed=14)], 3, channel=channel)
    check(gpu_ctx, [normal_map(h, w, np.uint8, seed=13)], [rough_map(h, w, np.uint8, seed=14)], 3, channel=channel)


@pytest.mark.parametrize("base", [0.0, 0.5, 1.0])
def test_constant_roughness(gpu_ctx, base):
    w, h = 64, 64
    for perceptual in (False, True):
        rec = check(gpu_ctx, [normal_map(h, w, np.uint8, seed=15)], base, 7, perceptual=perceptual)
        if base == 1.0:
            assert all(r["saturated"] > 0 for r in rec[0])
    flat = np.zeros((h, w, 4), np.float32)
    flat[..., 2] = 1.0
    _, after, rec = run(gpu_ctx, [flat], base, 7, signed_normals=True)
    for k, a in enumerate(after[0]):
        assert (a[..., 1].view(np.float32) == np.float32(base)).all()
        assert rec[0][k]["clamped"] == 0 and rec[0][k]["max_added"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_normals_and_roughness_in_one_surface(gpu_ctx, dtype):
    """x and y of a two-channel normal in red and green, the roughness in alpha"""
    w, h = 65, 31
    check(gpu_ctx, [normal_map(h, w, dtype, seed=16), normal_map(h, w, dtype, seed=17)], None, 7, channel=3,
          reconstruct_z=True, same=True, pad=3)


def test_pitches_with_a_gap(gpu_ctx):
    w, h = 33, 17
    for ndtype, rdtype, pad, rpad in ((np.uint8, np.float32, 5, 1), (np.float16, np.uint8, 1, 7), (np.float32, np.float16, 2, 3)):
        check(gpu_ctx, [normal_map(h, w, ndtype, seed=18)], [rough_map(h, w, rdtype, seed=19)], 6, pad=pad, rpad=rpad)


def test_degenerate_and_opposed_normals(gpu_ctx):
    w, h = 8, 8
    n = np.zeros((h, w, 4), np.float32)
    n[..., 2] = 1.0
    n[0, 0, :3] = np.nan
    n[0, 1, :3] = (np.inf, 0, 1)
    n[1, 0, :3] = (0, -np.inf, 0)
    n[1, 1, :3] = 0.0                                  # a level-1 texel of four degenerate normals: +z
    n[2:4, 2, 2] = -1.0                                # two down, two up: the mean is the zero vector
    n[4, 4:6, :3] = (1, 0, 0)
    n[5, 4:6, :3] = (-1, 0, 0)
    half = n.astype(np.float16)
    for maxv in (1.0, 0.18):
        for img in (n, half):
            rec = check(gpu_ctx, [img], 0.2, 4, signed_normals=True, max_variance=maxv)
            assert rec[0][0]["clamped"] >= 2
            assert rec[0][0]["max_added"] == int(np.float32(maxv).view(np.uint32))
    _, after, _ = run(gpu_ctx, [n], 0.2, 4, signed_normals=True, perceptual=False)
    level1 = after[0][0][..., 1].view(np.float32)
    assert level1[0, 0] == np.float32(0.2)             # the degenerate four
    assert level1[1, 1] == 1.0 and level1[2, 2] == 1.0  # alpha^2 + 1 saturates
    # the roughness rules: NaN, negative, above 1
    m = np.zeros((h, w, 4), np.float32)
    m[..., 1] = 0.5
    m[0, 0, 1], m[0, 1, 1], m[1, 0, 1], m[1, 1, 1] = np.nan, -3.0, 2.0, np.inf
    check(gpu_ctx, [n], [m], 4, signed_normals=True)
    check(gpu_ctx, [n], [m.astype(np.float16)], 4, signed_normals=True, perceptual=False)


def test_clamp_of_kaplanyan(gpu_ctx):
    w, h = 130, 70
    n = [normal_map(h, w, np.uint8, seed=20, strength=1.5)]
    rec = check(gpu_ctx, n, [rough_map(h, w, np.uint8, seed=21)], 8, variance_scale=2.0, max_variance=0.18)
    assert all(r["clamped"] > 0 for r in rec[0])
    cap = int(np.float32(np.float64(np.float32(2.0))*np.float64(np.float32(0.18))).view(np.uint32))
    assert all(r["max_added"] == cap for r in rec[0])
    free = check(gpu_ctx, n, [rough_map(h, w, np.uint8, seed=21)], 8)
    assert sum(r["clamped"] for r in free[0]) < sum(r["clamped"] for r in rec[0])
    check(gpu_ctx, n, 0.1, 8, variance_scale=0.0)


def test_identical_calls_return_identical_bits_and_the_time_answers(gpu_ctx):
    w, h = 130, 70
    n = [normal_map(h, w, np.uint8, seed=s) for s in (22, 23)]
    r = [rough_map(h, w, np.float32, seed=s) for s in (24, 25)]
    a = run(gpu_ctx, n, r, 8)
    ms = gpu_ctx.last_kernel_ms()
    assert ms > 0.0 and gpu_ctx.last_kernel_name() == "cfhip_spec_aa_texel_kernel"
    b = run(gpu_ctx, n, r, 8)
    assert all(x.tobytes() == y.tobytes() for la, lb in zip(a[1], b[1]) for x, y in zip(la, lb)) and a[2] == b[2]
    # on a stream of the caller's
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = run(gpu_ctx, n, r, 8, stream=s.cuda_stream)
    assert all(x.tobytes() == y.tobytes() for la, lc in zip(a[1], c[1]) for x, y in zip(la, lc)) and a[2] == c[2]


def test_host_convenience(gpu_ctx):
    w, h = 33, 17
    n, r = normal_map(h, w, np.uint8, seed=26), rough_map(h, w, np.uint8, seed=27)
    values, rec = gpu_ctx.specular_aa(n, r, 6, channel="b")
    want, wrec = R.specular_aa(n, r, 6, 2, R.PERCEPTUAL)
    assert all(v.tobytes() == x.tobytes() for v, x in zip(values, want)) and rec == wrec
    values, rec = gpu_ctx.specular_aa(n, 0.5, 3, perceptual=False, variance_scale=2.0, max_variance=0.18)
    want, wrec = R.specular_aa(n, 0.5, 3, 1, 0, 2.0, 0.18)
    assert all(v.tobytes() == x.tobytes() for v, x in zip(values, want)) and rec == wrec
    with pytest.raises(api.CfhipError):
        gpu_ctx.specular_aa(n, 0.5, 7)                 # beyond the chain


def build_pair(dim, w, h, depth, seed):
    """a normal texture (uint8, level 0 only) and a roughness texture (float32 level 0, Box chain) of one geometry"""
    normals, rough = Texture(dim, w, h, depth, 1), Texture(dim, w, h, depth, 1)
    faces = list(CubeFace) if dim == Dimension.Cube else [None]
    for d in range(max(depth, 1)):
        for f in faces:
            args = (0, d) if f is None else (f, 0, d)
            s = seed + 10*d + (int(f) if f is not None else 0)
            assert normals.set_image(normal_map(h, w, np.uint8, seed=s), *args)
            assert rough.set_image(np.clip(rough_map(h, w, np.uint8, seed=s).astype(np.float32)/255.0, 0, 1), *args)
    assert rough.generate_mipmaps(ResizeFilter.Box)
    return normals, rough, faces


@pytest.mark.parametrize("dim,depth", [(Dimension.Cube, 0), (Dimension.Dim2D, 3)])
def test_texture_equals_the_context_path(gpu_ctx, dim, depth):
    w, h = 64, 32
    normals, rough, faces = build_pair(dim, w, h, depth, seed=40)
    mips = rough.mip_level_count()
    assert mips == 7
    get = lambda t, f, m, d: t.get_image(m, d) if f is None else t.get_image(f, m, d)      # noqa: E731
    nbefore = {(d, f): get(normals, f, 0, d).copy() for d in range(max(depth, 1)) for f in faces}
    rbefore = {(m, d, f): get(rough, f, m, d).copy() for m in range(mips) for d in range(max(depth, 1)) for f in faces}
    assert rough.specular_aa_results() == []
    assert rough.specular_antialias(normals, channel="g", variance_scale=2.0, max_variance=0.18)
    records = rough.specular_aa_results()
    assert len(records) == (mips - 1)*max(depth, 1)*len(faces)
    assert [(r["mip"], r["depth"], r["face"]) for r in records] == sorted((r["mip"], r["depth"], r["face"]) for r in records)
    for d in range(max(depth, 1)):
        for fi, f in enumerate(faces):
            assert get(normals, f, 0, d).tobytes() == nbefore[(d, f)].tobytes()
            assert get(rough, f, 0, d).tobytes() == rbefore[(0, d, f)].tobytes()
            values, rec = gpu_ctx.specular_aa(nbefore[(d, f)], rbefore[(0, d, f)], mips, channel="g", variance_scale=2.0,
                                              max_variance=0.18)
            for m in range(1, mips):
                got, was = get(rough, f, m, d), rbefore[(m, d, f)]
                assert got.dtype == np.float32 and got[..., 1].tobytes() == values[m - 1].tobytes()
                assert got[..., [0, 2, 3]].tobytes() == was[..., [0, 2, 3]].tobytes()
                mine = [r for r in records if (r["mip"], r["depth"], r["face"]) == (m, d, fi)][0]
                assert (mine["clamped"], mine["saturated"]) == (rec[m - 1]["clamped"], rec[m - 1]["saturated"])
                assert np.float32(mine["max_added"]).view(np.uint32) == rec[m - 1]["max_added"]
    # the texture may be its own normal map: x and y in red and green, the roughness in alpha
    packed = Texture(dim, w, h, depth, 1)
    for d in range(max(depth, 1)):
        for f in faces:
            assert packed.set_image(nbefore[(d, f)], *((0, d) if f is None else (f, 0, d)))
    assert packed.generate_mipmaps(ResizeFilter.Box)
    assert packed.specular_antialias(packed, channel="a", reconstruct_z=True)
    d, f = max(depth, 1) - 1, faces[-1]
    values, _ = gpu_ctx.specular_aa(nbefore[(d, f)], nbefore[(d, f)], mips, channel="a", reconstruct_z=True)
    assert get(packed, f, 0, d).tobytes() == nbefore[(d, f)].tobytes()
    for m in range(1, mips):
        assert get(packed, f, m, d)[..., 3].tobytes() == values[m - 1].tobytes()
