#!/usr/bin/env python3
"""What specular anti-aliasing buys: the GGX distribution a mip level renders against the one
its level-0 footprint renders, with the plain roughness chain and with this pass.  On the CPU, through the numpy twin
(tests/spec_aa_ref.py), which the kernels match bit for bit.

Input: 256^2 height fields of smooth noise (white noise, three 3 x 3 box blurs, unit variance; seeds 1 and 2, both
axes wrapped) through Image.create_normal_map's formula, n = (dx, dy, 1) / len with dx = (left - right) * height / 2
and dy = (below - above) * height / 2, at height 0.5 and 2; a constant GGX alpha of 0.1, 0.3 and 0.6 (linear
encoding); levels 1, 2 and 4.
Reference: for a texel of level k and a half-vector h, the mean over the texel's level-0 footprint of D(n . h, alpha),
D(c, a) = a^2 / (pi ((c^2 (a^2 - 1)) + 1)^2), c clamped at 0 -- what supersampling would shade.
Plain chain: D(m . h, alpha) with m the renormalised mean normal (generate_mipmaps(normalize=...)): the roughness chain
of a constant is the constant.  This pass: D(m . h, alpha_k) with alpha_k the level the pass writes.
Four half-vectors: +z, and 10, 25 and 45 degrees off it towards +x, +y and (-x, -y).  The figure is the root of the
mean squared difference to the reference over the level's texels, the half-vectors and both seeds.  The tool fails if
a row does not improve.

    python tools/spec_aa_quality.py [--out profiles/spec_aa_quality.md]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SIZE = 256
HEIGHTS = (0.5, 2.0)
ALPHAS = (0.1, 0.3, 0.6)
LEVELS = (1, 2, 4)
SEEDS = (1, 2)


def height_field(n, seed):
    """(n, n) smooth noise of unit variance, wrapped"""
    f = np.random.default_rng(seed).standard_normal((n, n))
    for _ in range(3):
        f = sum(np.roll(f, (dy, dx), (0, 1)) for dy in (-1, 0, 1) for dx in (-1, 0, 1))/9.0
    return f/f.std()


def normals_of(field, height):
    """(n, n, 3) unit normals of a height field, Image.create_normal_map's formula with both axes wrapped"""
    dx = (np.roll(field, 1, 1) - np.roll(field, -1, 1))*height/2.0
    dy = (np.roll(field, -1, 0) - np.roll(field, 1, 0))*height/2.0
    v = np.stack([dx, dy, np.ones_like(dx)], -1)
    return v/np.sqrt((v*v).sum(-1, keepdims=True))


def ggx(c, a):
    c = np.maximum(c, 0.0)
    a2 = a*a
    return a2/(math.pi*((c*c)*(a2 - 1.0) + 1.0)**2)


def half_vectors():
    out = [np.array([0.0, 0.0, 1.0])]
    for deg, (x, y) in ((10, (1, 0)), (25, (0, 1)), (45, (-math.sqrt(0.5), -math.sqrt(0.5)))):
        s, c = math.sin(math.radians(deg)), math.cos(math.radians(deg))
        out.append(np.array([x*s, y*s, c]))
    return out


def box(a, k):
    """the mean over 2^k x 2^k footprints (SIZE is a power of two: no odd ends)"""
    s = 1 << k
    return a.reshape(a.shape[0]//s, s, a.shape[1]//s, s, *a.shape[2:]).mean((1, 3))


def rows():
    import spec_aa_ref as R
    for height in HEIGHTS:
        maps = [normals_of(height_field(SIZE, seed), height) for seed in SEEDS]
        for alpha in ALPHAS:
            err = {k: [0.0, 0.0, 0] for k in LEVELS}
            mean_alpha = {k: [] for k in LEVELS}
            for n in maps:
                stored = np.concatenate([n, np.zeros((SIZE, SIZE, 1))], -1).astype(np.float32)
                levels, _ = R.specular_aa(stored, alpha, max(LEVELS) + 1, 1, R.SIGNED_NORMALS)
                for k in LEVELS:
                    m = box(n, k)
                    m = m/np.sqrt((m*m).sum(-1, keepdims=True))
                    ak = levels[k - 1].astype(np.float64)
                    mean_alpha[k].append(ak.mean())
                    for h in half_vectors():
                        ref = box(ggx(n @ h, alpha), k)
                        err[k][0] += ((ggx(m @ h, alpha) - ref)**2).sum()
                        err[k][1] += ((ggx(m @ h, ak) - ref)**2).sum()
                        err[k][2] += ref.size
            for k in LEVELS:
                plain, ours = math.sqrt(err[k][0]/err[k][2]), math.sqrt(err[k][1]/err[k][2])
                yield height, alpha, k, float(np.mean(mean_alpha[k])), plain, ours


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = ["# Specular anti-aliasing: the distribution a level renders against its footprint's",
           "",
           "`tools/spec_aa_quality.py`, on the CPU through `tests/spec_aa_ref.py` (the kernels return its bits).  256x256",
           "height fields of smooth noise (two seeds) through `create_normal_map`'s formula at the given height; a constant",
           "GGX alpha (linear encoding, `variance_scale` 1, `max_variance` 1).  The reference is the box-filtered GGX",
           "distribution of level 0 under each texel, for four half-vectors (+z and 10, 25, 45 degrees off it).  `plain`:",
           "the renormalised mean normal with the unchanged alpha; `this pass`: the same normal with the alpha the pass",
           "writes.  RMSE over texels, half-vectors and seeds.",
           "",
           "| height | alpha | level | mean alpha written | RMSE plain | RMSE this pass | ratio |",
           "|---|---|---|---|---|---|---|"]
    worse = 0
    for height, alpha, k, written, plain, ours in rows():
        out.append("| %g | %g | %d | %.4f | %.4g | %.4g | %.2f |" % (height, alpha, k, written, plain, ours, ours/plain))
        worse += not ours < plain
    out += ["", "%d of %d rows improve." % (len(HEIGHTS)*len(ALPHAS)*len(LEVELS) - worse, len(HEIGHTS)*len(ALPHAS)*len(LEVELS))]
    text = "\n".join(out) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if worse:
        sys.exit("%d rows did not improve" % worse)


if __name__ == "__main__":
    main()
