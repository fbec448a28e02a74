"""bench.py --dump-outputs: a payload larger than the dump budget is written as the same seeded sample of its
blocks on every run, as float32 within 64 MB, each row the bytes of the block its index names."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_a_large_payload_is_dumped_as_a_fixed_sample_of_its_blocks(tmp_path):
    n = 3 * bench.DUMP_BLOCKS
    payload = torch.from_numpy(np.random.default_rng(5).integers(0, 256, n * 16, dtype=np.uint8))
    for d in ("a", "b"):
        bench.dump_payload(str(tmp_path / d), "bc7_payload", payload)
    got = np.load(tmp_path / "a" / "bc7_payload.npy")
    idx = np.load(tmp_path / "a" / "bc7_payload_block_index.npy")
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_BLOCKS, 16)
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(got, payload.numpy().reshape(-1, 16)[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(got, np.load(tmp_path / "b" / "bc7_payload.npy"))
    assert np.array_equal(idx, np.load(tmp_path / "b" / "bc7_payload_block_index.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
