"""The mip post-pass on the GPU (cfhip_mip_post_array_device, cfhip_alpha_coverage_device) against its numpy twin
(tests/mip_post_ref.py), byte for byte: the levels and the result records.  Level 0 is checked untouched by every call."""
import numpy as np
import pytest

import mip_post_ref as R
from cuttlefish_amd import CfhipError, CubeFace, Dimension, Format, ResizeFilter, Texture, Type, api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BOX, CATMULL = int(ResizeFilter.Box), int(ResizeFilter.CatmullRom)
THRESHOLDS = (0.5, 1/255, 1.0)


def content(kind, h, w, dtype, seed=0):
    """(h, w, 4) image of dtype whose alpha is: soft noise, a sparse binary mask, a pattern that thins out when averaged
    (the levels must go up), a dense mask that fills in (they must go down), a tie, hard-edged blocks, opaque, clear,
    or a smooth field"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    checker = np.where((x + y) & 1, 1.0, -1.0)
    a = {"noise": lambda: np.clip(rng.random((h, w))*1.4 - 0.2, 0, 1),
         "binary": lambda: (rng.random((h, w)) < 0.3).astype(np.float64),
         "thin": lambda: 0.45 + 0.4*checker,
         "fat": lambda: (rng.random((h, w)) < 0.7).astype(np.float64),
         # all or nothing: below 1 the count drops from every texel to none, a tie that goes to u, whose count is the
         # one at scale 1 -- rule 5 keeps the level
         "tie": lambda: 0.55 + 0.4*checker,
         # hard edges between plateaus four texels wide: a filter with negative lobes leaves [0, 1] there
         "blocks": lambda: np.kron((rng.random((h//4 + 1, w//4 + 1)) < 0.4).astype(np.float64), np.ones((4, 4)))[:h, :w],
         "opaque": lambda: np.ones((h, w)),
         "clear": lambda: np.zeros((h, w)),
         "blob": lambda: np.clip(0.5 + 0.9*(np.sin(x*0.9 + seed)*np.cos(y*0.7) + 0.3*np.sin(x*0.23 + y*0.31)), 0, 1)}[kind]()
    img = np.concatenate([rng.random((h, w, 3)), a[..., None]], -1)
    if dtype == np.uint8:
        return np.round(img*255).astype(np.uint8)
    return img.astype(dtype)


def chain_length(w, h):
    return int(np.floor(np.log2(max(w, h)))) + 1


def upload_level0(img, pad):
    """level 0 on the device, `pad` texels between its rows, all ones: alpha that would count if it were read"""
    h, w = img.shape[:2]
    buf = np.full((h, w + pad, 4), 255 if img.dtype == np.uint8 else 1, img.dtype)
    buf[:, :w] = img
    return torch.from_numpy(buf.view(np.uint8).reshape(h, -1).copy()).cuda(), buf.strides[0]


def gpu_chain(ctx, img, filt, levels=None):
    """the float32 levels 1.. that cfhip_generate_mips_device makes of img"""
    h, w = img.shape[:2]
    levels = levels or chain_length(w, h)
    src, pitch = upload_level0(img, 0)
    dsts = [torch.empty((max(1, h >> k), max(1, w >> k), 4), dtype=torch.float32, device="cuda") for k in range(1, levels)]
    ctx.generate_mips_device(src.data_ptr(), api.pixel_type_of(img), w, h, pitch, [d.data_ptr() for d in dsts], filter=filt)
    return [d.cpu().numpy() for d in dsts]


def run(ctx, level0s, chains, alpha_coverage=None, normalize=None, pad=0):
    """One call on uploaded copies: level0s[l] and chains[l] (its float32 levels) -> (the levels after the call, the
    records as a (layers, levels) structured array, or None without coverage)"""
    h, w = level0s[0].shape[:2]
    srcs = [upload_level0(im, pad) for im in level0s]
    before = [s.clone() for s, _ in srcs]
    dev = [[torch.from_numpy(np.ascontiguousarray(lv)).cuda() for lv in chain] for chain in chains]
    per = len(chains[0])
    res = torch.full((len(level0s)*per, 4), -1, dtype=torch.int32, device="cuda")
    ctx.mip_post_device([s.data_ptr() for s, _ in srcs], api.pixel_type_of(level0s[0]), w, h, srcs[0][1],
                        [[d.data_ptr() for d in c] for c in dev], alpha_coverage=alpha_coverage, normalize=normalize,
                        results=res.data_ptr() if alpha_coverage is not None else 0)
    for (s, _), b in zip(srcs, before):
        assert torch.equal(s, b), "level 0 was written"
    rec = res.cpu().numpy()
    if alpha_coverage is None:
        assert (rec == -1).all(), "the records were written without COVERAGE"
        rec = None
    else:
        rec = rec.view(api.MIP_POST_RESULT_DTYPE).reshape(len(level0s), per)
    return [[d.cpu().numpy() for d in c] for c in dev], rec


def flags_of(alpha_coverage, normalize):
    return (R.COVERAGE if alpha_coverage is not None else 0) | (R.NORMALIZE if normalize else 0) | \
        (R.SIGNED_NORMALS if normalize == "snorm" else 0)


def check(level0s, chains, got, rec, alpha_coverage=None, normalize=None, what=""):
    """the call's output against the twin's, layer by layer; -> the twin's `how` per layer"""
    hows = []
    for l, (level0, chain) in enumerate(zip(level0s, chains)):
        how = []
        want, wrec = R.post(level0, chain, flags_of(alpha_coverage, normalize), alpha_coverage or 0.5, info=how)
        hows.append(how)
        for k, (g, w_) in enumerate(zip(got[l], want), start=1):
            assert g.tobytes() == w_.tobytes(), (what, "layer", l, "level", k)
        for k, r in enumerate(wrec):
            g = rec[l, k]
            assert (R.bits(g["scale"]), int(g["target"]), int(g["count_before"]), int(g["count_after"])) == \
                (R.bits(r["scale"]), r["target"], r["count_before"], r["count_after"]), (what, "layer", l, "level", k + 1, g, r)
    return hows


CASES = [(64, 64, np.uint8, BOX, "noise", 0), (64, 64, np.float16, BOX, "binary", 0), (64, 64, np.float32, CATMULL, "blocks", 0),
         (64, 64, np.float32, BOX, "tie", 0),
         (67, 35, np.uint8, BOX, "fat", 3), (67, 35, np.float32, CATMULL, "blocks", 5), (67, 35, np.uint8, BOX, "blob", 0), (67, 35, np.float16, BOX, "thin", 1),
         (8, 2, np.float32, BOX, "noise", 0), (8, 2, np.uint8, BOX, "binary", 2),
         (256, 256, np.uint8, BOX, "noise", 0), (256, 256, np.float32, CATMULL, "thin", 7)]


@pytest.mark.parametrize("w,h,dtype,filt,kind,pad", CASES,
                         ids=["%dx%d-%s-%s-%s-pad%d" % (c[0], c[1], np.dtype(c[2]).name, "box" if c[3] == BOX else "catmull", c[4], c[5])
                              for c in CASES])
def test_chain_matches_twin(gpu_ctx, w, h, dtype, filt, kind, pad):
    level0 = content(kind, h, w, dtype, seed=w + h)
    chain = gpu_chain(gpu_ctx, level0, filt)
    assert [c.shape[:2] for c in chain] == [(max(1, h >> k), max(1, w >> k)) for k in range(1, chain_length(w, h))]
    if filt == CATMULL and kind != "thin":
        a = np.concatenate([c[..., 3].ravel() for c in chain])
        assert a.min() < 0 and a.max() > 1                 # the filter's overshoot is part of the case
    for t in THRESHOLDS:
        got, rec = run(gpu_ctx, [level0], [chain], alpha_coverage=t, pad=pad)
        check([level0], [chain], got, rec, alpha_coverage=t, what="t=%g" % t)
        for g, c, r in zip(got[0], chain, rec[0]):
            assert np.array_equal(g[..., :3], c[..., :3])
            if r["scale"] == 1:
                assert g.tobytes() == c.tobytes()


def test_a_one_texel_level0_has_no_chain_to_repair(gpu_ctx):
    src = torch.ones((1, 1, 4), dtype=torch.float32, device="cuda")
    lvl = torch.ones((1, 1, 4), dtype=torch.float32, device="cuda")
    res = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(CfhipError) as e:
        gpu_ctx.mip_post_device([src.data_ptr()], api.PixelType.RGBA32F, 1, 1, 16, [[lvl.data_ptr()]], alpha_coverage=0.5,
                                results=res.data_ptr())
    assert e.value.code == api.E_INVALID and "levels_count" in str(e.value)
    # the shortest chain there is: 2 x 1 and its 1 x 1 level
    level0 = content("noise", 1, 2, np.float32, 3)
    level0[..., 3] = (0.9, 0.2)
    chain = [np.full((1, 1, 4), 0.3, np.float32)]
    got, rec = run(gpu_ctx, [level0], [chain], alpha_coverage=0.5)
    assert check([level0], [chain], got, rec, alpha_coverage=0.5) == [["u"]] and rec[0, 0]["target"] == 1


def test_hand_built_levels_clamps_nan_and_negative_alpha(gpu_ctx):
    from test_mip_post_ref import clamp_cases
    cases = clamp_cases()
    level0s = [c[1] for c in cases]
    chains = [[c[2]] for c in cases]
    # a level of NaN, negative, infinite and ordinary alpha under a half-covered level 0
    half = content("opaque", 16, 16, np.float32)
    half[8:, :, 3] = 0.0
    odd = content("noise", 8, 8, np.float32, 5)
    odd[0, :, 3] = np.nan
    odd[1, :, 3] = -0.75
    odd[2, :4, 3] = np.inf
    odd[2, 4:, 3] = -np.inf
    odd[3, :, 3] = np.float32(np.uint32(0x7FA00001).view(np.float32))      # a signalling NaN with a payload
    odd[4:, :, 3] *= 0.4
    level0s.append(half)
    chains.append([odd])
    got, rec = run(gpu_ctx, level0s, chains, alpha_coverage=0.5)
    hows = check(level0s, chains, got, rec, alpha_coverage=0.5)
    assert [h[0] for h in hows[:4]] == [c[5] for c in cases]
    assert [float(r["scale"]) for r in rec[:4, 0]] == [c[4] for c in cases]
    assert rec[4, 0]["scale"] > 1 and rec[4, 0]["target"] == 32
    a = got[4][0][..., 3]
    assert (a[0] == 1).all() and (a[1] < 0).all() and (a[2, :4] == 1).all() and (a[2, 4:] == -np.inf).all() and (a[3] == 1).all()


def test_18_layers_in_one_call_equal_18_calls(gpu_ctx):
    kinds = ("thin", "fat", "opaque", "binary", "noise", "clear")
    level0s = [content(kinds[i % 6], 64, 64, np.uint8, seed=i) for i in range(18)]        # 6 faces x 3 elements
    chains = [gpu_chain(gpu_ctx, im, BOX) for im in level0s]
    got, rec = run(gpu_ctx, level0s, chains, alpha_coverage=0.5)
    check(level0s, chains, got, rec, alpha_coverage=0.5)
    scales = rec["scale"]
    assert (scales > 1).any() and (scales < 1).any() and (scales == 1).any()
    assert (scales[0] > 1).any() and (scales[1] < 1).any() and (scales[2] == 1).all() and (scales[5] == 1).all()
    for l in range(18):
        one, rec1 = run(gpu_ctx, [level0s[l]], [chains[l]], alpha_coverage=0.5)
        assert rec1.tobytes() == rec[l:l + 1].tobytes(), l
        for k in range(len(chains[l])):
            assert one[0][k].tobytes() == got[l][k].tobytes(), (l, k)
            if scales[l, k] == 1:
                assert got[l][k].tobytes() == chains[l][k].tobytes(), (l, k)


def normal_level0(h, w, signed, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(h, w, 3))
    v /= np.sqrt((v*v).sum(-1, keepdims=True))
    if not signed:
        v = v*0.5 + 0.5
    return np.concatenate([v, np.clip(rng.random((h, w, 1))*1.4 - 0.2, 0, 1)], -1).astype(np.float32)


@pytest.mark.parametrize("normalize", ["unorm", "snorm"])
def test_normals(gpu_ctx, normalize):
    signed = normalize == "snorm"
    level0 = normal_level0(35, 67, signed, 11)
    chain = gpu_chain(gpu_ctx, level0, BOX)
    # degenerate texels, written straight into a level: the zero vector, an all-NaN texel, an infinite component
    chain[1][0, 0, :3] = 0.0 if signed else 0.5
    chain[1][0, 1, :3] = np.nan
    chain[1][0, 2, :3] = (np.inf, 0.25, 0.5)
    chain[1][0, 3] = np.nan                                 # alpha too: it must come back with its bits
    got, rec = run(gpu_ctx, [level0], [chain], normalize=normalize, pad=2)
    check([level0], [chain], got, None, normalize=normalize)
    plus_z = [0.0, 0.0, 1.0] if signed else [0.5, 0.5, 1.0]
    assert got[0][1][0, :4, :3].tolist() == [plus_z]*4
    for g, c in zip(got[0], chain):
        assert g[..., 3].tobytes() == c[..., 3].tobytes()           # alpha untouched
        dec = g[..., :3].astype(np.float64) if signed else g[..., :3].astype(np.float64)*2 - 1
        assert np.abs(np.sqrt((dec*dec).sum(-1)) - 1).max() <= 2.0**-23
    shortened = np.sqrt(((chain[3][..., :3].astype(np.float64)*(1 if signed else 2) - (0 if signed else 1))**2).sum(-1))
    assert shortened.min() < 0.9                            # the averaged normals were in need of it
    # fused with coverage = the two flags in two calls
    both, rec_both = run(gpu_ctx, [level0], [chain], alpha_coverage=0.5, normalize=normalize)
    check([level0], [chain], both, rec_both, alpha_coverage=0.5, normalize=normalize)
    cov, rec_cov = run(gpu_ctx, [level0], [chain], alpha_coverage=0.5)
    two, _ = run(gpu_ctx, [level0], [cov[0]], normalize=normalize)
    assert rec_both.tobytes() == rec_cov.tobytes() and (rec_cov["scale"] != 1).any()
    assert [a.tobytes() for a in both[0]] == [a.tobytes() for a in two[0]]


def test_alpha_coverage_device(gpu_ctx):
    images = [content("noise", 35, 67, np.uint8, 1), content("blob", 64, 64, np.float16, 2), content("noise", 2, 8, np.float32, 3),
              content("binary", 256, 256, np.float32, 4), content("noise", 1, 1, np.uint8, 5)]
    images[2][0, :3, 3] = (np.nan, -1.0, np.inf)
    pads = (3, 1, 0, 5, 2)
    up = [upload_level0(im, p) for im, p in zip(images, pads)]
    surfaces = [dict(pixels=t.data_ptr(), pixel_type=api.pixel_type_of(im), width=im.shape[1], height=im.shape[0], row_pitch_bytes=p)
                for im, (t, p) in zip(images, up)]
    for thr in THRESHOLDS:
        for scale in (1.0, 1.5):
            counts = torch.full((len(images) + 1,), -1, dtype=torch.int32, device="cuda")
            gpu_ctx.alpha_coverage_device(surfaces, thr, counts.data_ptr(), scale)
            got = counts.cpu().numpy()
            with np.errstate(invalid="ignore"):
                want = [int(np.count_nonzero(R.alpha_of(im)*np.float32(scale) >= np.float32(thr))) for im in images]
            assert got[:-1].tolist() == want and got[-1] == -1, (thr, scale)
            assert want == [R.coverage(im, thr, scale) for im in images]
    assert 0 < want[0] < 35*67
    assert gpu_ctx.alpha_coverage(images[0], 0.5) == R.coverage(images[0], 0.5)
    assert gpu_ctx.alpha_coverage(images[1][:, 3:40], 0.25, 1.5) == R.coverage(images[1][:, 3:40], 0.25, 1.5)


def test_identical_calls_launch_counts_and_timing(gpu_ctx):
    level0s = [content(k, 67, 35, np.float16, seed=i) for i, k in enumerate(("thin", "fat", "noise"))]
    chains = [gpu_chain(gpu_ctx, im, CATMULL) for im in level0s]
    a, rec_a = run(gpu_ctx, level0s, chains, alpha_coverage=0.5, normalize="unorm")
    b, rec_b = run(gpu_ctx, level0s, chains, alpha_coverage=0.5, normalize="unorm")
    assert rec_a.tobytes() == rec_b.tobytes()
    assert [x.tobytes() for c in a for x in c] == [x.tobytes() for c in b for x in c]
    assert gpu_ctx.last_kernel_ms() > 0 and gpu_ctx.last_kernel_name() == "cfhip_mip_post_count_kernel"
    # the launches of a call do not depend on its layers or levels
    launches = []
    for layers, kw in ((1, dict(alpha_coverage=0.5)), (3, dict(alpha_coverage=0.5, normalize="snorm")), (3, dict(normalize="unorm"))):
        gpu_ctx.profile_begin()
        run(gpu_ctx, level0s[:layers], chains[:layers], **kw)
        ms, n = gpu_ctx.profile_end()
        assert ms > 0
        launches.append(n)
    assert launches == [15, 15, 1]


def textures(kind):
    """-> (make(): a fresh texture with its level-0 images set, the level-0 images in [depth][face] order)"""
    if kind == "2d":
        dim, w, h, depth, faces = Dimension.Dim2D, 64, 48, 0, 1
    elif kind == "cube":
        dim, w, h, depth, faces = Dimension.Cube, 32, 32, 0, 6
    else:
        dim, w, h, depth, faces = Dimension.Dim2D, 32, 16, 3, 1
    kinds = ("thin", "fat", "noise", "binary", "opaque", "blob")
    images = [[content(kinds[(d*faces + f) % 6], h, w, np.uint8, seed=d*faces + f) for f in range(faces)] for d in range(max(depth, 1))]

    def make():
        t = Texture(dim, w, h, depth)
        for d, row in enumerate(images):
            for f, im in enumerate(row):
                assert t.set_image(im, CubeFace(f), 0, d) if dim == Dimension.Cube else t.set_image(im, 0, d)
        return t
    return make, images


@pytest.mark.parametrize("kind", ["2d", "cube", "array"])
def test_texture_generate_mipmaps_with_alpha_coverage(kind):
    make, images = textures(kind)
    plain, off, post = make(), make(), make()
    assert plain.generate_mipmaps(ResizeFilter.Box)
    assert off.generate_mipmaps(ResizeFilter.Box, alpha_coverage=None, normalize=None)
    assert post.generate_mipmaps(ResizeFilter.Box, alpha_coverage=0.5)
    levels = plain.mip_level_count()
    assert levels == post.mip_level_count() == off.mip_level_count() > 3
    cube = plain.dimension() == Dimension.Cube
    results = post.mip_post_results()
    assert len(results) == len(images)*len(images[0]) and plain.mip_post_results() == off.mip_post_results() == []
    moved = 0
    for d, row in enumerate(images):
        for f, level0 in enumerate(row):
            def image(t, mip):
                return t.get_image(CubeFace(f), mip, d) if cube else t.get_image(mip, d)
            chain = [image(plain, m) for m in range(1, levels)]
            for m in range(levels):
                assert image(off, m).tobytes() == image(plain, m).tobytes()         # keywords off: today's images
            assert image(post, 0).tobytes() == level0.tobytes()
            want, wrec = R.post(level0, chain, R.COVERAGE, 0.5)
            for m in range(1, levels):
                assert image(post, m).tobytes() == want[m - 1].tobytes(), (d, f, m)
            got = results[d*len(row) + f]
            assert [(R.bits(g["scale"]), g["target"], g["count_before"], g["count_after"]) for g in got] == \
                [(R.bits(r["scale"]), r["target"], r["count_before"], r["count_after"]) for r in wrec]
            moved += sum(r["scale"] != 1 for r in wrec)
    assert moved > 0
    assert post.convert(Format.BC3, Type.UNorm)


def test_texture_custom_mips_normals_and_volumes():
    from cuttlefish_amd import CustomMipImage, image_index
    make, images = textures("2d")
    custom = {image_index(2, 0): CustomMipImage(content("fat", 12, 16, np.uint8, 9))}
    plain, post = make(), make()
    assert plain.generate_mipmaps(ResizeFilter.Box, Texture.allMipLevels, custom)
    assert post.generate_mipmaps(ResizeFilter.Box, Texture.allMipLevels, custom, alpha_coverage=0.5, normalize="unorm")
    chain = [plain.get_image(m) for m in range(1, plain.mip_level_count())]
    want, wrec = R.post(images[0][0], chain, R.COVERAGE | R.NORMALIZE, 0.5)
    for m, w_ in enumerate(want, start=1):
        assert post.get_image(m).tobytes() == w_.tobytes(), m
    assert [g["count_after"] for g in post.mip_post_results()[0]] == [r["count_after"] for r in wrec]
    assert post.convert(Format.BC5, Type.UNorm)
    vol = Texture(Dimension.Dim3D, 8, 8, 4)
    for d in range(4):
        assert vol.set_image(content("noise", 8, 8, np.uint8, d), 0, d)
    assert vol.generate_mipmaps(ResizeFilter.Box, alpha_coverage=0.5) is False
    assert vol.generate_mipmaps(ResizeFilter.Box, normalize="snorm") is False
    assert vol.generate_mipmaps(ResizeFilter.Box) and vol.convert(Format.BC1_RGB, Type.UNorm)
