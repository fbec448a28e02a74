"""Writes tests/golden/pvrtc_photos.npz: power-of-two crops of the photographs that ship with scikit-learn (china.jpg,
flower.jpg) and matplotlib (grace_hopper.jpg), at fixed positions, for the PVRTC1 tests and tools/bench_pvrtc.py.

  rgb   (6, 128, 128, 4) uint8   six 128 x 128 RGB crops, alpha 255
  rgba  (2, 128, 128, 4) uint8   two of the crops with another crop's luma (Rec. 601, integer) as alpha

The PVRTC quality ladder was tuned on these crops: they are not held-out data.
Run: python tests/golden/make_pvrtc_photos.py"""
import os

import numpy as np
from PIL import Image


def _load(path):
    return np.asarray(Image.open(path).convert("RGB"))


def main():
    import matplotlib
    import sklearn
    sk = os.path.join(os.path.dirname(sklearn.__file__), "datasets", "images")
    mpl = os.path.join(os.path.dirname(matplotlib.__file__), "mpl-data", "sample_data")
    china, flower = _load(os.path.join(sk, "china.jpg")), _load(os.path.join(sk, "flower.jpg"))
    grace = _load(os.path.join(mpl, "grace_hopper.jpg"))
    spots = [(china, 40, 60), (china, 200, 300), (flower, 100, 150), (flower, 250, 400), (grace, 60, 200),
             (grace, 300, 150)]
    rgb = np.empty((len(spots), 128, 128, 4), np.uint8)
    for i, (im, y, x) in enumerate(spots):
        rgb[i, ..., :3] = im[y:y + 128, x:x + 128]
        rgb[i, ..., 3] = 255
    luma = lambda c: (c[..., :3].astype(np.int64) @ np.array([299, 587, 114]) + 500) // 1000
    rgba = np.stack([rgb[1].copy(), rgb[4].copy()])
    rgba[0, ..., 3] = luma(rgb[2])
    rgba[1, ..., 3] = luma(rgb[5])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pvrtc_photos.npz")
    np.savez_compressed(out, rgb=rgb, rgba=rgba)
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    main()
