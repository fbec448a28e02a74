"""The numpy twin of the mip post-pass (tests/mip_post_ref.py) against the laws its definitions imply, on inputs where
the laws are not vacuous: a noise mask, a smooth field, an RGBA8 soft mask and a binary mask through a box chain, opaque
and clear images, and hand-built levels for the two clamps."""
import numpy as np
import pytest

import mip_post_ref as R

THRESHOLDS = (0.5, 1/255, 1.0)
ULP1 = 2.0**-23                       # one float32 ulp at 1


def rgba(alpha: np.ndarray) -> np.ndarray:
    h, w = alpha.shape
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([x/max(w - 1, 1), y/max(h - 1, 1), np.full((h, w), 0.25)], -1)
    if alpha.dtype == np.uint8:
        return np.concatenate([np.round(rgb*255).astype(np.uint8), alpha[..., None]], -1)
    return np.concatenate([rgb.astype(alpha.dtype), alpha[..., None]], -1)


def inputs():
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:64, 0:64]
    blob = np.sin(x*0.9)*np.cos(y*0.7) + 0.3*np.sin(x*0.23 + y*0.31)
    return {
        "noise": rgba(np.clip(rng.random((64, 64))*1.4 - 0.2, 0, 1).astype(np.float32)),
        "smooth": rgba(np.clip(0.5 + 0.9*blob, 0, 1).astype(np.float32)),
        "soft8": rgba(np.clip(np.round((0.55 + 0.4*np.where((x + y) & 1, 1, -1))*255), 0, 255).astype(np.uint8)),
        "binary": rgba((rng.random((64, 64)) < 0.3).astype(np.float32)),
        "opaque": rgba(np.ones((64, 64), np.float32)),
        "clear": rgba(np.zeros((64, 64), np.float32)),
    }


@pytest.fixture(scope="module")
def runs():
    """every (input, threshold): level 0, its box chain, the levels after the pass, the records, how each was chosen"""
    out = []
    for name, level0 in inputs().items():
        chain = R.box_chain(level0, 7)
        for t in THRESHOLDS:
            how = []
            after, rec = R.post(level0, chain, R.COVERAGE, t, info=how)
            out.append((name, t, level0, chain, after, rec, how))
    return out


def test_counts_never_move_away_from_the_target(runs):
    for name, t, level0, chain, after, rec, how in runs:
        c0 = R.coverage(level0, t)
        for k, (before, cur, r) in enumerate(zip(chain, after, rec), start=1):
            n = before.shape[0]*before.shape[1]
            assert r["target"] == (c0*n + 64*64//2)//(64*64)
            assert r["count_before"] == R.coverage(before, t)
            # the record's count is the count of the scale, and of the level as it was written
            assert r["count_after"] == R.coverage(before, t, r["scale"]) == R.coverage(cur, t), (name, t, k)
            assert abs(r["count_after"] - r["target"]) <= abs(r["count_before"] - r["target"]), (name, t, k)
            assert r["scale"] == 1 or r["count_after"] != r["count_before"], (name, t, k)
            assert np.float32(R.S_MIN) <= r["scale"] <= np.float32(R.S_MAX)
            assert np.array_equal(cur[..., :3], before[..., :3])
            if r["scale"] == 1:
                assert cur.tobytes() == before.tobytes()


def test_the_scale_is_the_extremum_over_bit_patterns(runs):
    seen = set()
    for name, t, level0, chain, after, rec, how in runs:
        for before, r, h in zip(chain, rec, how):
            s, T = r["scale"], r["target"]
            cnt = lambda b: R.count(before[..., 3], R.fl(b), t)        # noqa: E731
            b = R.bits(s)
            seen.add(("up" if s > 1 else "down" if s < 1 else "stay", h))
            if h == "u" and s > 1:
                assert s <= R.S_MAX and cnt(b - 1) < T <= cnt(b)
                assert abs(cnt(b) - T) <= abs(cnt(b - 1) - T)
            elif h == "d" and s > 1:
                assert cnt(b) < T <= cnt(b + 1) and abs(cnt(b) - T) < abs(cnt(b + 1) - T)
            elif h == "d" and s < 1:
                assert s >= R.S_MIN and cnt(b) <= T < cnt(b + 1)
                assert abs(cnt(b) - T) < abs(cnt(b + 1) - T)
            elif h == "u" and s < 1:
                assert cnt(b - 1) <= T < cnt(b) and abs(cnt(b) - T) <= abs(cnt(b - 1) - T)
            elif h == "max":                       # no scale up to S_MAX reaches the target
                assert s == R.S_MAX and r["count_before"] < cnt(b) < T
            elif h == "min":                       # no scale down to S_MIN comes down to it
                assert s == R.S_MIN and r["count_before"] > cnt(b) > T
            else:
                assert s == 1, (name, t, h)
    dirs = {d for d, _ in seen}
    assert dirs == {"up", "down", "stay"}, seen
    # both candidates get chosen, above 1 and below
    assert {("up", "u"), ("down", "d")} <= seen, seen


def test_opaque_and_clear_images_come_back_as_they_were(runs):
    for name, t, level0, chain, after, rec, how in runs:
        if name in ("opaque", "clear"):
            assert all(r["scale"] == 1 for r in rec), (name, t)
            assert [a.tobytes() for a in after] == [c.tobytes() for c in chain]


def clamp_cases():
    """(name, level 0, one hand-built 8 x 8 level, threshold, the scale expected, how)"""
    full = rgba(np.ones((16, 16), np.float32))
    none = rgba(np.zeros((16, 16), np.float32))
    low = np.full((8, 8), 0.01, np.float32)
    high = np.full((8, 8), 3.0, np.float32)
    mixed_low, mixed_high = low.copy(), high.copy()
    mixed_low[:3] = 0.2                # S_MAX lifts these over 0.5, the others stay below: 24 of a target of 64
    mixed_high[:3] = 1.0               # S_MIN takes these below 0.5, the others stay above: 40 over a target of 0
    return [("low", full, rgba(low), 0.5, 1.0, "max=1"), ("mixed low", full, rgba(mixed_low), 0.5, 4.0, "max"),
            ("high", none, rgba(high), 0.5, 1.0, "min=1"), ("mixed high", none, rgba(mixed_high), 0.5, 0.25, "min")]


def test_both_clamps():
    for name, level0, level, t, scale, how in clamp_cases():
        info = []
        after, rec = R.post(level0, [level], R.COVERAGE, t, info=info)
        r = rec[0]
        assert info == [how] and r["scale"] == np.float32(scale), (name, r, info)
        assert abs(r["count_after"] - r["target"]) <= abs(r["count_before"] - r["target"])
        if scale == 1.0:
            assert after[0].tobytes() == level.tobytes()
        else:
            assert r["count_after"] != r["count_before"] and r["count_after"] == R.coverage(after[0], t)
            assert after[0][..., 3].max() <= 1.0


def test_nan_and_negative_alpha_never_count():
    a = np.array([[np.nan, -1.0, -np.inf, np.inf], [0.5, 0.49999997, -0.0, 2.0]], np.float32)
    assert R.count(a, 1.0, 0.5) == 3 and R.count(a, 4.0, 0.5) == 4 and R.count(a, 0.25, 0.5) == 2
    out = R.scale_alpha(rgba(a), 2.0)[..., 3]
    assert out.tobytes() == np.array([[1.0, -2.0, -np.inf, 1.0], [1.0, 0.99999994, -0.0, 1.0]], np.float32).tobytes()


def normal_field(h, w, seed):
    rng = np.random.default_rng(seed)
    v = (rng.integers(-512, 513, (h, w, 3))/512.0).astype(np.float32)       # 2u - 1 is exact on this grid
    alpha = rng.random((h, w)).astype(np.float32)
    return np.concatenate([v, alpha[..., None]], -1)


def test_normals_are_unit_length_and_keep_alpha():
    signed = normal_field(33, 17, 3)
    signed[0, 0, :3] = 0.0
    unsigned = signed.copy()
    unsigned[..., :3] = signed[..., :3]*0.5 + 0.5
    assert np.array_equal(unsigned[..., :3]*2 - 1, signed[..., :3])
    s_out = R.post(signed, [signed], R.NORMALIZE | R.SIGNED_NORMALS)[0][0]
    u_out = R.post(unsigned, [unsigned], R.NORMALIZE)[0][0]
    for got, dec in ((s_out, s_out[..., :3].astype(np.float64)), (u_out, u_out[..., :3].astype(np.float64)*2 - 1)):
        assert got[..., 3].tobytes() == signed[..., 3].tobytes()
        assert np.abs(np.sqrt((dec*dec).sum(-1)) - 1.0).max() <= ULP1
    # the zero vector is +z in both storages
    assert s_out[0, 0, :3].tolist() == [0.0, 0.0, 1.0] and u_out[0, 0, :3].tolist() == [0.5, 0.5, 1.0]
    # the two storages hold the same normals: half an ulp of each store apart at the most
    assert np.abs((u_out[..., :3].astype(np.float64)*2 - 1) - s_out[..., :3]).max() <= 2.0**-24 + 2.0**-25
    # direction kept: a vector already of unit length on the grid stays
    axis = np.zeros((1, 1, 4), np.float32)
    axis[0, 0] = (0.0, -1.0, 0.0, 0.3)
    assert R.normalize(axis, True).tobytes() == axis.tobytes()


def test_degenerate_normals_become_plus_z():
    bad = np.zeros((1, 4, 4), np.float32)
    bad[0, 1, :3] = np.nan
    bad[0, 2, :3] = (np.inf, 0.5, 0.5)
    bad[0, 3, :3] = (3e38, 3e38, 3e38)          # finite in double: an ordinary vector
    bad[..., 3] = (0.1, np.nan, 0.3, 0.4)
    s_out = R.normalize(bad, True)
    assert s_out[0, :3, :3].tolist() == [[0.0, 0.0, 1.0]]*3
    assert np.allclose(s_out[0, 3, :3], 3**-0.5)
    assert s_out[..., 3].tobytes() == bad[..., 3].tobytes()
    u_out = R.normalize(bad, False)
    assert u_out[0, 1:3, :3].tolist() == [[0.5, 0.5, 1.0]]*2
    # (0, 0, 0) in unsigned storage is the vector (-1, -1, -1)
    assert np.allclose(u_out[0, 0, :3].astype(np.float64)*2 - 1, -(3**-0.5))


def test_fused_equals_two_calls():
    level0 = inputs()["noise"]
    chain = R.box_chain(level0, 5)
    both, rec = R.post(level0, chain, R.COVERAGE | R.NORMALIZE, 0.5)
    cov, rec2 = R.post(level0, chain, R.COVERAGE, 0.5)
    two, _ = R.post(level0, cov, R.NORMALIZE)
    assert rec == rec2 and [a.tobytes() for a in both] == [a.tobytes() for a in two]
