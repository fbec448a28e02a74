"""The numpy twin of specular anti-aliasing (tests/spec_aa_ref.py) against itself and against values worked out by
hand: what the definition promises before any kernel is compared with it."""
import math

import numpy as np
import pytest

import spec_aa_ref as R

SIZES = [(3, 3), (5, 3), (7, 5), (95, 40), (1, 64)]


def flat(h, w, dtype=np.float32):
    """+z everywhere in the unorm storage"""
    n = np.zeros((h, w, 4), np.float64)
    n[..., :2] = 0.5
    n[..., 2] = 1.0
    return np.round(n*255).astype(np.uint8) if dtype == np.uint8 else n.astype(dtype)


def bumpy(h, w, seed, strength=1.0):
    """random unit normals around +z, signed float32 storage"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.normal(0, strength, (h, w, 2)), np.ones((h, w, 1)), np.zeros((h, w, 1))], -1)
    v[..., :3] /= np.linalg.norm(v[..., :3], axis=-1, keepdims=True)
    return v.astype(np.float32)


def rough_map(h, w, seed, dtype=np.float32):
    r = np.random.default_rng(seed).random((h, w, 4))
    return np.round(r*255).astype(np.uint8) if dtype == np.uint8 else r.astype(dtype)


@pytest.mark.parametrize("flags", [0, R.PERCEPTUAL])
@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32])
def test_flat_normals_keep_the_roughness(flags, dtype):
    values, records = R.specular_aa(flat(12, 20, dtype), 0.5, 5, flags=flags)
    assert [v.shape for v in values] == [(6, 10), (3, 5), (1, 2), (1, 1)]
    for v, rec in zip(values, records):
        assert (v == np.float32(0.5)).all()
        # 8 bits cannot store +z (128 / 255 is not a half): the normals are equal but tilted, their Q30 components are
        # rounded by up to 2^-31 each, and the mean's length misses 1 by that much -- far below half an ulp of 0.25f
        added = float(np.uint32(rec.pop("max_added")).view(np.float32))
        assert added == 0.0 if dtype != np.uint8 else 0.0 <= added <= 2.0**-29
        assert rec == dict(clamped=0, saturated=0, reserved=0)


@pytest.mark.parametrize("flags", [R.SIGNED_NORMALS, R.SIGNED_NORMALS | R.PERCEPTUAL])
def test_a_pair_of_tilted_normals_has_the_closed_form(flags):
    for s in (0.1, 0.5, 0.9):
        c = math.sqrt(1.0 - s*s)
        n = np.zeros((2, 2, 4), np.float32)
        n[:, 0, :3] = (s, 0, c)
        n[:, 1, :3] = (-s, 0, c)
        r = 0.3
        (v,), (rec,) = R.specular_aa(n, r, 2, flags=flags)
        alpha = r*r if flags & R.PERCEPTUAL else r
        # Level 0 is quantised, so the closed form is taken at the c and the alpha^2 the sums hold: the Q30 value of c
        # (within 2^-31 of the float32 c renormalised) and the Q32 value of alpha^2 (within 2^-33).  In double, before
        # the value is stored, the two agree to 1e-12: a dozen operations of 2^-53 each on values below 1.
        qx, qy, qz, qa = R.moments(n, r, 1, flags)
        assert qx.sum() == 0 and qy.sum() == 0 and (qz == qz[0, 0]).all() and (qa == qa[0, 0]).all()
        cq, a2q = int(qz[0, 0])/R.Q30, int(qa[0, 0])/R.Q32
        assert abs(cq - float(np.float32(c))/math.hypot(float(np.float32(s)), float(np.float32(c)))) <= 2.0**-31
        assert abs(a2q - alpha*alpha) <= 2.0**-33 + 1e-7      # r itself is a float32
        a2 = R.finish_a2(qx.sum(keepdims=True).reshape(1, 1), qy.sum().reshape(1, 1), qz.sum().reshape(1, 1),
                         qa.sum().reshape(1, 1), np.array([[4]]), 1.0, 1.0)[0]
        want = a2q + (1.0 - cq*cq)/(cq*(3.0 - cq*cq))
        assert abs(float(a2[0, 0]) - want) <= 1e-12, (s, float(a2[0, 0]), want)
        # the stored float32 is that value's root (the fourth root with PERCEPTUAL), rounded once
        root = math.sqrt(float(a2[0, 0]))
        assert v[0, 0] == np.float32(math.sqrt(root) if flags & R.PERCEPTUAL else root)
        assert rec["clamped"] == 0 and rec["saturated"] == 0


def test_opposed_normals_give_max_variance():
    n = np.zeros((2, 2, 4), np.float32)
    n[0, :, 2] = 1.0
    n[1, :, 2] = -1.0
    for maxv in (0.18, 0.5):
        (v,), (rec,) = R.specular_aa(n, 0.0, 2, flags=R.SIGNED_NORMALS, max_variance=maxv)
        assert v[0, 0] == np.float32(np.sqrt(np.float64(np.float32(maxv))))
        assert rec == dict(clamped=1, saturated=0, max_added=int(np.float32(maxv).view(np.uint32)), reserved=0)
    (v,), (rec,) = R.specular_aa(n, 0.0, 2, flags=R.SIGNED_NORMALS, variance_scale=2.0)
    assert v[0, 0] == 1.0 and rec["saturated"] == 1 and rec["max_added"] == int(np.float32(2.0).view(np.uint32))


@pytest.mark.parametrize("w,h", SIZES)
def test_hierarchical_sums_are_the_footprint_sums(w, h):
    rng = np.random.default_rng(w*100 + h)
    q = rng.integers(-2**30, 2**30, (h, w), dtype=np.int64)
    cur = q
    for k in range(1, R.chain_levels(w, h)):
        cur = R.child_sums(cur)
        wk, hk = R.level_dims(w, h, k)
        assert cur.shape == (hk, wk)
        direct = R.direct_sums(q, k)
        counts = np.outer(R.footprint_counts(h, k), R.footprint_counts(w, k))
        covered = 0
        for y in range(hk):
            for x in range(wk):
                x0, x1 = x << k, (w if x == wk - 1 else (x + 1) << k)
                y0, y1 = y << k, (h if y == hk - 1 else (y + 1) << k)
                want = sum(int(v) for v in q[y0:y1, x0:x1].ravel())       # Python integers
                assert int(cur[y, x]) == want == int(direct[y, x]), (k, x, y)
                assert int(counts[y, x]) == (x1 - x0)*(y1 - y0)
                covered += (x1 - x0)*(y1 - y0)
        assert covered == w*h                          # every level-0 texel in exactly one texel of the level
    assert R.direct_sums(np.ones((3, 3), np.int64), 1).tolist() == [[9]]


@pytest.mark.parametrize("w,h", SIZES + [(33, 17)])
def test_never_below_the_rms_alpha_and_equal_to_it_without_variance(w, h):
    n, r = bumpy(h, w, 7), rough_map(h, w, 8)
    count = R.chain_levels(w, h)
    for flags in (R.SIGNED_NORMALS, R.SIGNED_NORMALS | R.PERCEPTUAL):
        values, _ = R.specular_aa(n, r, count, channel=2, flags=flags)
        plain, records = R.specular_aa(n, r, count, channel=2, flags=flags, variance_scale=0.0)
        direct, _ = R.specular_aa(n, r, count, channel=2, flags=flags, hierarchical=False)
        qa = R.moments(n, r, 2, flags)[3]
        for k, (v, p, d) in enumerate(zip(values, plain, direct), start=1):
            assert v.tobytes() == d.tobytes()
            assert (v >= p).all() and (v > p).any()
            mean = R.direct_sums(qa, k).astype(np.float64)/(np.outer(R.footprint_counts(h, k), R.footprint_counts(w, k))*R.Q32)
            rms = np.sqrt(mean)
            want = (np.sqrt(rms) if flags & R.PERCEPTUAL else rms).astype(np.float32)
            assert p.tobytes() == want.tobytes()
            assert records[k - 1]["max_added"] == 0 and records[k - 1]["saturated"] == 0


def test_degenerate_normals_act_as_plus_z():
    bad = np.zeros((4, 4, 4), np.float32)
    bad[0, 0, :3] = np.nan
    bad[0, 1, :3] = (np.inf, 0, 1)
    bad[0, 2, :3] = (0, -np.inf, 0)
    bad[0, 3, :3] = (np.nan, 0, 1)
    bad[1, :, 2] = 1.0                                 # a row of real +z; the rest is the zero vector
    good = np.zeros((4, 4, 4), np.float32)
    good[..., 2] = 1.0
    for flags in (R.SIGNED_NORMALS, R.SIGNED_NORMALS | R.RECONSTRUCT_Z):
        q = R.quantise_normals(bad, flags)
        if not flags & R.RECONSTRUCT_Z:
            assert all((a == b).all() for a, b in zip(q, R.quantise_normals(good, flags)))
        a, _ = R.specular_aa(bad, 0.25, 3, flags=flags)
        if not flags & R.RECONSTRUCT_Z:
            b, _ = R.specular_aa(good, 0.25, 3, flags=flags)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # two-channel normals: the blue is ignored, (0, 0) is +z, x^2 + y^2 > 1 leaves z = 0
    two = np.zeros((1, 2, 4), np.float32)
    two[0, 0] = (0, 0, -5, 0)
    two[0, 1] = (3, 4, 9, 0)
    qx, qy, qz = R.quantise_normals(two, R.SIGNED_NORMALS | R.RECONSTRUCT_Z)
    assert (qx[0, 0], qy[0, 0], qz[0, 0]) == (0, 0, 2**30)
    assert (qx[0, 1], qy[0, 1], qz[0, 1]) == (round(0.6*2**30), round(0.8*2**30), 0)
    # the unorm storage of the zero vector is (0.5, 0.5, 0.5); 8-bit storage cannot hold it, float can
    half = np.full((2, 2, 4), 0.5, np.float32)
    assert all((a == b).all() for a, b in zip(R.quantise_normals(half, 0), R.quantise_normals(good[:2, :2], R.SIGNED_NORMALS)))


def test_roughness_rules():
    r = np.array([np.nan, -1.0, -0.0, 0.0, 0.5, 1.0, 1.5, np.inf, -np.inf])
    assert R.quantise_roughness(r, 0).tolist() == [0, 0, 0, 0, 2**30, 2**32, 2**32, 2**32, 0]
    assert R.quantise_roughness(r, R.PERCEPTUAL).tolist() == [0, 0, 0, 0, 2**28, 2**32, 2**32, 2**32, 0]
    n = flat(2, 2)
    m = np.zeros((2, 2, 4), np.float32)
    m[..., 3] = [[np.nan, -3.0], [2.0, 1.0]]
    (v,), _ = R.specular_aa(n, m, 2, channel=3, flags=0)
    assert v[0, 0] == np.float32(math.sqrt(0.5))
    with pytest.raises(ValueError):
        R.specular_aa(n, m, 3)
    with pytest.raises(ValueError):
        R.specular_aa(n, m, 1)
    with pytest.raises(ValueError):
        R.specular_aa(n, m, 2, channel=4)


def test_decoding():
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 64, 4)
    d = R.decode(u8)
    assert d.dtype == np.float64 and (d == (u8.astype(np.float64)/255.0).astype(np.float32)).all()
    h = np.array([[[0.1, -2.5, 65504.0, np.inf]]], np.float16)
    assert (R.decode(h) == h.astype(np.float64)).all()
    with pytest.raises(TypeError):
        R.decode(np.zeros((1, 1, 4), np.float64))


def test_records():
    n, r = bumpy(40, 56, 3, strength=2.0), rough_map(40, 56, 4)
    count = R.chain_levels(56, 40)
    values, records = R.specular_aa(n, r, count, channel=0, flags=R.SIGNED_NORMALS | R.PERCEPTUAL, variance_scale=2.0,
                                    max_variance=0.18)
    free, free_rec = R.specular_aa(n, r, count, channel=0, flags=R.SIGNED_NORMALS | R.PERCEPTUAL)
    assert len(records) == count - 1 and all(tuple(rec) == R.FIELDS for rec in records)
    cap = np.float32(np.float64(np.float32(2.0))*np.float64(np.float32(0.18)))
    # a lower limit is met by at least the texels that meet a higher one
    assert any(rec["clamped"] for rec in records)
    assert all(a["clamped"] >= b["clamped"] for a, b in zip(records, free_rec))
    for v, rec in zip(values, records):
        assert 0 <= rec["clamped"] <= v.size and 0 <= rec["saturated"] <= v.size and rec["reserved"] == 0
        assert rec["max_added"] <= int(cap.view(np.uint32))
        if rec["clamped"]:
            assert rec["max_added"] == int(cap.view(np.uint32))
    # strong bumps on a rough surface reach alpha^2 = 1 without the clamp
    assert any(rec["saturated"] for rec in free_rec)
    assert all(float(np.uint32(rec["max_added"]).view(np.float32)) > 0 for rec in free_rec)
