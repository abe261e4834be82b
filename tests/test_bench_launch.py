"""bench.py's multi-rank control flow, end to end on CPU (first-lease insurance: the 8-GPU runs are the driver's and cannot be
debugged).  F3DGS_BENCH_STUB=1 replaces the op by a few torch operations and RCCL by gloo; everything else is the real file: the
re-launch under torch.distributed.run, the refusal rules, the exchange through dp.py, every diagnostic leg, the ONE JSON line
relayed from rank 0.  No number in these lines is a measurement ("data": "stub")."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=420):
    env = dict(os.environ, F3DGS_BENCH_STUB="1", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(lines) == 1, f"expected ONE JSON line from rank 0, got {len(lines)}:\n{p.stdout[-2000:]}"
    return json.loads(lines[0])


def test_two_ranks_relaunch_and_relay_one_line():
    d = _run("--gpus", "2", "--steps", "2", "--warmup", "1", "--full")
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["data"] == "stub"
    assert d["scaling"] == "weak" and d["higher_is_better"] is True and d["unit"] == "Mpix/s" and d["value"] > 0
    assert "dp2" in d["config"]["parallelism"] and "workload" in d["config"]
    b = d["dp_breakdown"]
    for k in ("compute_only_ms", "comm_only_ms", "comm_only_direct_ms", "bytes_per_rank", "comm_algbw_GBps", "train_step_allreduce_full_adam_ms",
              "train_step_sharded_optimizer_ms", "two_views_per_gpu_ms_per_step", "two_views_per_gpu_mpix_s"):
        assert k in b and b[k] is not None, (k, b)
    assert b["bytes_per_rank"] == 1500 * (59 + 8) * 4
    # the labels come from the library's options and the line carries the exact-fp32 figure beside the default
    assert d["options"]["bwd_bf16"] == -1 and "bf16" in d["dtype"] and d["blend_backward_contraction"] == "bf16 two-term" and d["ms_per_step_fp32_exact"] > 0
    assert d["roofline"]["kernel"] in ("render_bwd", "render_fwd") and d["roofline_whole_step"]["views_per_gpu_and_step"] == 1


def test_views_per_iter_line_is_strong_scaling_and_counts_views_per_gpu():
    d = _run("--gpus", "2", "--steps", "2", "--warmup", "1", "--views-per-iter", "4", "--full")
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["views_breakdown"]["views_per_rank"] == 2
    w = d["roofline_whole_step"]
    # one GPU moves the bytes of the TWO views it renders per step
    assert w["views_per_gpu_and_step"] == 2 and w["algorithmic_bytes"] % 2 == 0
    assert abs(w["frac"] - w["algorithmic_bytes"] / (d["ms_per_step"] * 1e-3) / 1e9 / 8000.0) < 1e-12


def test_comm_only_sweeps_the_collective_settings():
    d = _run("--gpus", "2", "--steps", "2", "--warmup", "1", "--comm-only")
    assert d["n_gpus"] == 2 and d["unit"] == "ms" and d["bytes_per_rank"] == 1500 * (59 + 8) * 4
    assert set(d["by_setting"]) >= {"NCCL_ALGO=Ring", "NCCL_ALGO=Tree", "NCCL_ALGO=Ring,NCCL_PROTO=Simple"}
    assert all(("ms" in v) or ("error" in v) for v in d["by_setting"].values())
    assert d["direct_all_to_all_plus_all_gather"]["ms"] > 0


def test_asking_for_more_gpus_than_ranks_is_refused():
    env = dict(os.environ, F3DGS_BENCH_STUB="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert p.returncode != 0 and "WORLD_SIZE=1" in (p.stderr + p.stdout)


def test_plain_line_is_the_headline_only(tmp_path):
    """Without --full the line carries the headline and nothing that needs runs of its own; --steps is the timed step count."""
    d = _run("--gpus", "1", "--steps", "3", "--warmup", "2")
    assert d["steps"] == 3 and d["warmup"] == 2 and d["full"] is False and d["steps_run_before_the_timed_region"] == 2 + 2 * 3
    assert d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["value"] > 0 and d["ms_per_step"] > 0
    assert "bf16" in d["dtype"] and d["metric"].startswith("rendered Mpix/s")
    for k in ("roofline", "roofline_whole_step", "stage_ms", "step_ms", "fp32_exact", "dp_breakdown", "cpu_baseline"):
        assert k not in d, k
    assert d["dumped_outputs"] is None


def test_dump_outputs_are_float_bounded_and_repeatable(tmp_path):
    import numpy as np
    runs = []
    for n in range(2):
        out = tmp_path / f"run{n}"
        d = _run("--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out))
        files = sorted(os.listdir(out))
        assert files == sorted(f"{name}.npy" for name in d["dumped_outputs"]) and "grad_means3D.npy" in files
        assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10 ** 6
        arrays = {f: np.load(out / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        runs.append(arrays)
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f


def test_dump_outputs_samples_what_does_not_fit(tmp_path):
    """At the headline size the whole output is ~0.6 GB: the same seeded pixels / rows of every array, within the budget."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    P, C, H, W = 400_000, 32, 540, 960
    images = {"color": torch.rand(3, H, W), "feature_map": torch.rand(C, H, W), "depth": torch.rand(1, H, W)}
    rows = {"radii": torch.arange(P, dtype=torch.int32), "grad_shs": torch.rand(P, 16, 3), "grad_semantic_feature": torch.rand(P, 1, C)}
    names = [bench.dump_outputs(str(tmp_path / f"d{n}"), images, rows) for n in range(2)]
    assert names[0] == names[1] == sorted([*images, *rows])
    total = sum(os.path.getsize(tmp_path / "d0" / f"{k}.npy") for k in names[0])
    assert 0.9 * bench.DUMP_BUDGET_BYTES < total <= 64 * 10 ** 6
    a = {k: np.load(tmp_path / "d0" / f"{k}.npy") for k in names[0]}
    b = {k: np.load(tmp_path / "d1" / f"{k}.npy") for k in names[0]}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    k_px = a["color"].shape[1]
    assert a["feature_map"].shape == (C, k_px) and a["depth"].shape == (1, k_px) and k_px < H * W
    idx = a["radii"].astype(np.int64)                    # radii = row index here: the sample is sorted and without repeats
    assert np.all(np.diff(idx) > 0) and len(idx) < P
    assert np.array_equal(a["grad_shs"], rows["grad_shs"].numpy()[idx])
