"""bench.py's --gpus contract: N ranks are launched by the script itself when no launcher
ran it, and a launcher's WORLD_SIZE must agree with --gpus (VERDICT r4 "next" #1)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_check_world_rules():
    assert bench.check_world(1, {}) == "run"
    assert bench.check_world(2, {}) == "launch"
    assert bench.check_world(8, {"WORLD_SIZE": "8"}) == "run"
    assert bench.check_world(1, {"WORLD_SIZE": "1"}) == "run"
    with pytest.raises(SystemExit):
        bench.check_world(1, {"WORLD_SIZE": "2"})  # the driver's launcher, --gpus left at 1
    with pytest.raises(SystemExit):
        bench.check_world(4, {"WORLD_SIZE": "2"})
    with pytest.raises(SystemExit):
        bench.check_world(0, {})


def test_launch_command():
    cmd = bench.launch_ranks(4, ["--gpus", "4", "--steps", "3"])
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-5:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "3"]


def _run(args, extra_env=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def test_gpus2_self_launches_two_ranks():
    """`python bench.py --gpus 2` (no launcher) runs two ranks: the line says n_gpus 2,
    and the MAX over ranks saw rank 1's value (gloo on this GPU-less host)."""
    r = _run(["--gpus", "2", "--dry-run", "--cpu-baseline", "off"], {"LLFE_BENCH_SHARE_GPU": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dry_run"] is True
    assert d["max_over_ranks_probe"] == 1.0
    assert d["config"]["parallelism"] == "replicas x2 (host-side shard, no collective)"
    assert d["config"]["global_batch"] == 1024


def test_world_size_mismatch_fails_before_gpu():
    r = _run(["--gpus", "1", "--dry-run"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "must agree" in r.stderr


def test_gpus_more_than_visible_fails():
    # (one GPU visible by the environment; with no readable kfd topology at all the parent
    # leaves the check to the ranks)
    r = _run(["--gpus", "64", "--dry-run"], {"HIP_VISIBLE_DEVICES": "0"})
    assert r.returncode != 0
    assert "GPUs are visible" in r.stderr


@pytest.mark.gpu
def test_gpus2_real_run_on_one_gpu():
    """The whole bench, self-launched at --gpus 2, both ranks sharing cuda:0 (the box has
    one GPU): one line, n_gpus 2, a value from both ranks' images."""
    r = _run(["--gpus", "2", "--full", "--batch", "16", "--steps", "2", "--warmup", "1", "--cpu-baseline", "off",
              "--per-class-steps", "0", "--e2e-host-steps", "0", "--e2e-png-steps", "0", "--e2e-jpeg-steps", "0"],
             {"LLFE_BENCH_SHARE_GPU": "1"}, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0
    assert d["config"]["global_batch"] == 32
    assert d["config"]["parallelism"].startswith("replicas x2")
    # the --full legs its arguments leave on ran on both ranks: the steps one batch at a
    # time with the kernel timings, the isolated-kernel step, served_batcher
    assert d["full"] is True and d["value_one_batch_at_a_time"] > 0
    assert d["served_batcher"]["value"] > 0 and len(d["served_batcher"]["per_rank"]) == 2
    assert d["kernels"]["k_kmeans"]["avg_ms"] > 0 and d["kernels"]["k_kmeans"]["isolated_ms"] > 0


def test_dump_outputs_layout(tmp_path):
    """--dump-outputs: one row per image, float32 / float64 only, -1 in unused slots."""
    import numpy as np

    from low_level_feature_extraction_amd.backend import ImageFeatures

    recs = [ImageFeatures(np.array([[1, 2, 3], [4, 5, 6]], np.uint8), np.array([7, 9]), 16, 2.5, 300_000_001, 77,
                          [{"type": "circle", "x": 1, "y": 2, "width": 3, "height": 4, "border_radius": 0.5,
                            "area": 9.25}], 3, 8, 6, ("#010203", "#0a0b0c", ["#ffffff", "", ""]), "High"),
            ImageFeatures(np.array([[9, 9, 9]], np.uint8), np.array([1]), 1, 0.0, 0, 0, [], 0, 8, 6,
                          ("#090909", "#090909", ["", "", ""]), "Low")]
    bench.dump_outputs(str(tmp_path / "d"), recs, ("colors", "shapes", "shadows"))
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert set(got) == {"centers_rgb", "counts", "n_unique", "compactness", "palette_rgb", "shadow_sum",
                        "shadow_count", "shadow_level", "n_contours", "n_shapes", "shapes"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["centers_rgb"].tolist() == [[[1, 2, 3], [4, 5, 6]], [[9, 9, 9], [-1, -1, -1]]]
    assert got["counts"].tolist() == [[7, 9], [1, -1]]
    assert got["shadow_sum"].tolist() == [300_000_001, 0]  # (past 2^24: float64)
    assert got["shadow_level"].tolist() == [2, 0]
    assert got["palette_rgb"][0].tolist() == [[1, 2, 3], [10, 11, 12], [255, 255, 255], [-1] * 3, [-1] * 3]
    assert got["n_shapes"].tolist() == [1, 0]
    assert got["shapes"].tolist() == [[0, 3, 1, 2, 3, 4, 0.5, 9.25]]
    # features not asked for leave no file
    bench.dump_outputs(str(tmp_path / "c"), recs, ("shadows",))
    assert sorted(os.listdir(tmp_path / "c")) == ["shadow_count.npy", "shadow_level.npy", "shadow_sum.npy"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path, backend):
    """A plain run (no --full): --steps timed steps, the secondary legs null, and
    --dump-outputs holds what the last timed step (seed + steps - 1) returned."""
    import numpy as np

    from low_level_feature_extraction_amd import synth

    B, H, W, seed, steps = 6, 135, 240, 77, 3
    d = tmp_path / "dump"
    r = _run(["--gpus", "1", "--batch", str(B), "--height", str(H), "--width", str(W), "--preprocessing", "none",
              "--seed", str(seed), "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(d),
              "--e2e-host-steps", "2"], timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "--e2e-host-steps only take effect with --full" in r.stderr  # (the leg stays off: e2e_host is None)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["full"] is False and line["value"] > 0
    # (both are rounded in the line: value to 0.01 images/s, ms_per_step to 0.001 ms)
    assert line["ms_per_step"] == pytest.approx(B / line["value"] * 1e3, rel=1e-3, abs=1e-3)
    for k in ("value_one_batch_at_a_time", "served_batcher", "per_class", "cpu_baseline", "e2e_host", "e2e_png",
              "e2e_jpeg", "roofline", "roofline_stencil"):
        assert line[k] is None, k
    imgs = synth.synth_batch(B, H, W, seed=seed, device="cuda:0", index_base=0)
    exp = backend.process(imgs, ("colors", "shapes", "shadows"), seed=seed + steps - 1, index_base=0)
    exp_dir = tmp_path / "exp"
    bench.dump_outputs(str(exp_dir), exp, ("colors", "shapes", "shadows"))
    assert sorted(os.listdir(d)) == sorted(os.listdir(exp_dir))
    for f in os.listdir(exp_dir):
        assert np.array_equal(np.load(d / f), np.load(exp_dir / f)), f
    # ... and not the step before it: the noise and k-means seeds follow the step's seed
    prev = backend.process(imgs, ("colors", "shapes", "shadows"), seed=seed + steps - 2, index_base=0)
    prev_dir = tmp_path / "prev"
    bench.dump_outputs(str(prev_dir), prev, ("colors", "shapes", "shadows"))
    assert any(not np.array_equal(np.load(d / f), np.load(prev_dir / f)) for f in os.listdir(prev_dir))


def test_visible_gpus_from_kfd_topology_without_hip(tmp_path):
    """The launching parent counts GPUs from sysfs (no HIP runtime in the parent)."""
    nodes = tmp_path / "nodes"
    for i, simds in enumerate([0, 1024, 1024, 0, 1024]):  # 2 CPU nodes, 3 GPUs
        (nodes / str(i)).mkdir(parents=True)
        (nodes / str(i) / "properties").write_text(f"cpu_cores_count 8\nsimd_count {simds}\nmax_waves_per_simd 8\n")
    assert bench.visible_gpus(env={}, sysfs=str(nodes)) == 3
    assert bench.visible_gpus(env={"HIP_VISIBLE_DEVICES": "0,1"}, sysfs=str(nodes)) == 2
    assert bench.visible_gpus(env={}, sysfs=str(tmp_path / "absent")) == 0
