"""bench.py end to end on the GPU box: the N-rank flow launched the way the driver launches N = 1
-- plain `python bench.py --gpus N` -- must start its own ranks, and the strong-scaling / C5
self-checks must actually compare bytes.  On a one-GPU box the ranks share the device through
the BENCH_DIST_BACKEND=gloo test hook (the data path is the same code; only the wire differs)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=900, extra_env=None):
    env = dict(os.environ)
    env.update(extra_env or {})
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    if torch.cuda.device_count() < 2:
        env["BENCH_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(1200)
def test_bench_gpus2_self_launches_and_reports_strong_scaling(hip_lib):
    line = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--size", "1024", "--no-cpu-baseline", "--full"])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    assert [p["rank"] for p in line["per_rank"]] == [0, 1]
    assert all(p["kernel_ms"] > 0 for p in line["per_rank"])
    st = line["strong_scaling"]
    assert st["scaling"] == "strong" and st["value"] > 0
    assert st["block_rows_per_rank"] == [128, 128]
    assert st["sharded_equals_local"]["equal"] is True
    assert st["sharded_equals_local"]["bytes_compared"] == 256*256*16
    assert set(st["phases_ms_max_over_ranks"]) == {"scatter", "encode", "gather"}


@pytest.mark.timeout(1800)
def test_bench_gpus8_weak_line_and_row_split_at_the_node_size(hip_lib):
    """`python bench.py --gpus 8` as the driver runs it on the 8-GPU node (SCALE): here the ranks share the
    visible devices through the gloo hook, so what is checked is the flow -- rendezvous, barriers, max over
    ranks, ONE JSON line from rank 0 -- and the 8-way block-row split of the strong-scaling leg (512 x 512:
    128 block rows, 16 per rank), byte-compared with the local encode."""
    line = _run(["--gpus", "8", "--steps", "2", "--warmup", "1", "--size", "512", "--no-cpu-baseline", "--full"],
                timeout=1500)
    assert line["n_gpus"] == 8 and line["scaling"] == "weak" and line["value"] > 0
    assert [p["rank"] for p in line["per_rank"]] == list(range(8))
    st = line["strong_scaling"]
    assert "error" not in st, st
    assert st["block_rows_per_rank"] == [16]*8
    assert st["sharded_equals_local"]["equal"] is True
    assert st["sharded_equals_local"]["bytes_compared"] == 128*128*16


@pytest.mark.timeout(1800)
def test_bench_c5_at_eight_ranks(hip_lib):
    """C5's texture sharding at the node size: 16 textures of 256 x 256 over 8 ranks (2 each), gathered to
    rank 0 and compared with local re-encodes of textures owned by ranks 0, 1 and 7."""
    line = _run(["--config", "c5", "--gpus", "8", "--textures", "16", "--tex-size", "256", "--steps", "1", "--full"],
                timeout=1500)
    chk = line["sharded_equals_local"]
    assert line["n_gpus"] == 8 and chk["equal"] is True
    assert {c["owner_rank"] for c in chk["textures_checked"]} == {0, 1, 7}
    assert [p["textures"] for p in line["per_rank"]] == [2]*8


@pytest.mark.timeout(1200)
def test_bench_c5_checks_textures_at_one_and_two_ranks(hip_lib):
    one = _run(["--config", "c5", "--gpus", "1", "--textures", "4", "--tex-size", "256", "--steps", "1", "--full"])
    chk = one["sharded_equals_local"]
    assert chk["equal"] is True and len(chk["textures_checked"]) >= 2
    two = _run(["--config", "c5", "--gpus", "2", "--textures", "8", "--tex-size", "256", "--steps", "1", "--full"])
    chk = two["sharded_equals_local"]
    assert two["n_gpus"] == 2 and chk["equal"] is True
    assert {c["owner_rank"] for c in chk["textures_checked"]} == {0, 1}
    assert all(c["equal"] for c in chk["textures_checked"])


@pytest.mark.timeout(600)
def test_a_stuck_strong_scaling_leg_cannot_take_the_weak_line_down(hip_lib):
    """The strong-scaling leg is an extra: with its watchdog set to fire at once, the job still prints
    exactly one line, exit code 0, with the weak-scaling value and an error note in place of the leg."""
    line = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--size", "1024", "--no-cpu-baseline", "--full"],
                extra_env={"BENCH_STRONG_TIMEOUT_S": "0.01"})
    assert line["n_gpus"] == 2 and line["value"] > 0 and len(line["per_rank"]) == 2
    st = line["strong_scaling"]
    assert "error" in st or st.get("value", 0) > 0


@pytest.mark.timeout(600)
def test_strict_mode_reports_a_failed_strong_leg_in_the_exit_status(hip_lib):
    """BENCH_STRONG_STRICT=1: still exactly one line with the weak value, exit status 3 when the leg timed out."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update({"BENCH_STRONG_TIMEOUT_S": "0.001", "BENCH_STRONG_STRICT": "1"})
    if torch.cuda.device_count() < 2:
        env["BENCH_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
                        "--size", "512", "--no-cpu-baseline", "--full"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=500, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["value"] > 0
    if "error" in line["strong_scaling"]:
        assert r.returncode != 0


@pytest.mark.timeout(1200)
def test_headline_line_carries_the_regression_gate_and_the_tolerance_level(hip_lib):
    """Round-5 ADVICE: nothing gated a drop of the headline against the previous round's record -- the line now says
    whether it holds 0.90 x that record (`regression_gate`), and this test fails when it does not.  `tolerance` names
    the lowest level whose gap to the bound is within north_star's 0.1 dB on both photograph groups and its measured
    throughput on the same tile (round-5 VERDICT item 3)."""
    line = _run(["--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-second-tile", "--full"])
    # (the tolerance leg encodes another level into the benchmark's payload buffer: the end-to-end leg that follows must
    # still be compared with the HEADLINE level's payload)
    assert line["end_to_end"]["rgba8"]["payload_equals_device_path"] is True
    assert line["end_to_end"]["rgba32f_bottom_up"]["payload_equals_device_path"] is True
    prev = line["vs_previous_round"]
    if prev is not None:
        assert int(prev["record"][7:9]) < 6, prev          # never this round's own record
        assert line["regression_gate"]["ok"], (line["value"], prev)
    tol = line["tolerance"]
    assert tol["target_db"] == 0.1 and tol["gap_db_normal_high_highest"] is not None
    assert tol["lowest_level_within_target"] in ("Normal", "High", "Highest")
    assert tol["mpixels_per_s"] >= 50.0                   # north_star's throughput at the compliant level
    k = ["Normal", "High", "Highest"].index(tol["lowest_level_within_target"])
    assert all(g[k] <= 0.1 for g in tol["gap_db_normal_high_highest"].values())


@pytest.mark.timeout(900)
def test_bench_config3_line(hip_lib):
    """BASELINE config 3 through bench.py (round-5 VERDICT item 1: the roofline line of --config c3 names the kernel)"""
    line = _run(["--config", "c3", "--size", "1536", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--full"])
    assert line["config"]["format"] == "ASTC_6x6" and line["config"]["quality"] == 3
    assert line["unit"] == "Mpixels/s" and line["value"] > 50.0 and line["dtype"] == "u8"
    r = line["roofline"]
    assert r["kernel"] == "cfhip_astc_encode_kernel" and r["bound"] == "hbm" and 0 < r["frac"] < 1
    assert r["algorithmic_bytes_per_launch"] == 1536*1536*4 + 256*256*16
    # the 0.1 dB view at C3's level: stated in the line, from the committed quality table (no level of 6x6 is inside)
    t = line["tolerance"]
    assert t["target_db"] == 0.1 and set(t["gap_db_normal_high_highest"]) == {"a", "b"}
    within = all(t["gap_db_normal_high_highest"][g][1] <= 0.1 for g in ("a", "b"))
    assert t["this_level_within_target"] == within


@pytest.mark.timeout(600)
def test_plain_run_times_the_headline_alone_and_dumps_its_last_step(gpu_ctx, tmp_path):
    """Without --full the line holds the headline alone, timed over exactly --steps launches; --dump-outputs writes
    the payload of the last timed step, which is the library's encode of the same seeded tile."""
    import numpy as np
    from cuttlefish_amd import Format, Type, make_params, synth
    line = _run(["--steps", "3", "--warmup", "1", "--size", "1024", "--dump-outputs", str(tmp_path)])
    assert line["steps"] == 3 and line["roofline"]["launches"] == 3 and line["ms_per_step"] > 0
    assert line["value"] > 0 and line["unit"] == "Mpixels/s" and line["dtype"] == "u8" and line["higher_is_better"]
    assert line["cpu_baseline"] is None and "valu_issue" not in line["roofline"]
    assert not {"vs_previous_round", "tolerance", "second_tile", "end_to_end", "strong_scaling"} & set(line)
    got = np.load(tmp_path / "bc7_payload.npy")
    idx = np.load(tmp_path / "bc7_payload_block_index.npy")
    assert got.dtype == np.float32 and got.shape == (256 * 256, 16)
    assert idx.dtype == np.float64 and np.array_equal(idx, np.arange(256 * 256))
    ref = gpu_ctx.encode([synth.photo(1024, 1024, seed=1)], make_params(Format.BC7, Type.UNorm, 2))[0]
    assert np.array_equal(got.reshape(-1), ref.astype(np.float32))
