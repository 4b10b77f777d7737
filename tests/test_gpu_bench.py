"""bench.py's multi-rank path as the driver uses it: `bench.py --gpus N`
run directly spawns N rank processes itself (torch.distributed.run, one process per GPU, before
the parent touches the GPU) and rank 0 prints ONE JSON line with n_gpus == N and config 4's
per-chunk workload.  On the one-GPU box the ranks share device 0 (GSR_BENCH_SHARE_GPU=1: gloo for
the barriers and the MAX of the elapsed time; the driver's 8-GPU runs use RCCL)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_bench_gpus2_spawns_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env["GSR_BENCH_SHARE_GPU"] = "1"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--full", "--gaussians", "200000", "--profile-steps", "1", "--train-steps", "2", "--no-config5", "--no-street",
           "--no-cpu-baseline", "--no-config3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=380, env=env, cwd=REPO)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["steps"] == 3 and d["warmup"] == 1
    c4 = d["config4"]
    assert c4["n_gpus"] == 2 and c4["value"] > 0 and len(c4["train_step_ms_per_rank"]) == 2
    assert all(v > 0 for v in c4["train_step_ms_per_rank"])


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_bench_gpus2_trains_one_chunk_per_rank():
    """Config 4 as the product runs it (scripts/full_train.py:171-232): with --gpus 2 every rank trains
    its own synthetic street chunk (seed = rank) through the train_single.py loop (here 300 iterations
    of a small chunk); the line reports the aggregate chunk-iterations/s over the job's wall clock and
    every rank's chunk wall clock."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env["GSR_BENCH_SHARE_GPU"] = "1"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--full", "--gaussians", "100000", "--profile-steps", "1", "--train-steps", "0", "--no-config5", "--no-street",
           "--no-cpu-baseline", "--chunk-iterations", "300", "--chunk-size", "384", "--chunk-positions", "8",
           "--chunk-truth", "100000", "--chunk-init", "40000"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=380, env=env, cwd=REPO)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, r.stdout[-3000:]
    ch = json.loads(lines[0])["config4"]["chunks"]
    assert ch["n_gpus"] == 2 and len(ch["chunk_wall_s_per_rank"]) == 2
    assert all(w > 0 for w in ch["chunk_wall_s_per_rank"]) and ch["job_wall_s"] >= max(ch["chunk_wall_s_per_rank"])
    assert abs(ch["chunk_iterations_per_s"] - 2 * 300 / ch["job_wall_s"]) <= 0.01 * ch["chunk_iterations_per_s"] + 0.02
    assert ch["P_final_rank0"] > 0


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_bench_plain_run_is_lean_and_dumps_last_step(tmp_path):
    """A plain run (no --full) prints the headline line only -- none of the diagnostics or legs that take
    runs of their own -- and --dump-outputs writes what its last timed step returned: float32 arrays,
    whole where they fit their share of the budget (here all but the SH gradient), and equal to the
    same frame rendered in this process from the same seeded inputs (radii exactly; the image within
    1e-5: a pixel blends a few hundred fp32 terms of magnitude <= 1 in depth order; the sampled SH
    gradient within 1e-4 relative L2, twice the bar the gradients meet against the oracle: two runs
    differ only in the order of the backward's atomic sums)."""
    import numpy as np
    import torch

    import bench
    P, W, H = 300_000, 320, 200  # 48 P SH-gradient elements: more than the budget leaves them
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--gaussians", str(P), "--width", str(W), "--height", str(H), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env, cwd=REPO)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["value"] > 0 and d["unit"] == "Mpix/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["metric"].startswith("fwd+bwd Mpix/s")
    assert abs(d["value"] - W * H / d["ms_per_step"] / 1e3) <= 2e-3 * d["value"]
    for k in ("roofline", "stages_ms", "train_step", "config4", "config5", "config3_proxy", "street_frame",
              "coarse_debug", "cpu_baseline", "cpu_baseline_torch", "psnr_vs_oracle", "valu_roofline"):
        assert k not in d, k
    names = {"color": (3, H, W), "invdepth": (1, H, W), "radii": (P,), "grad_means3D": (P, 3),
             "grad_means2D": (P, 3), "grad_opacities": (P, 1), "grad_scales": (P, 3), "grad_rotations": (P, 4)}
    files = sorted(f.name for f in out.iterdir())
    assert files == sorted([n + ".npy" for n in names] + ["grad_shs.npy"])
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64_000_000
    got = {f.name[:-4]: np.load(f) for f in out.iterdir()}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    for n, shape in names.items():
        assert got[n].shape == shape, (n, got[n].shape)
    # the SH gradient (P x 16 x 3) is over its share: the seeded sample of its elements
    plan = bench.dump_plan({**{n: int(np.prod(s)) for n, s in names.items()}, "grad_shs": P * 48})
    assert got["grad_shs"].shape == (plan["grad_shs"],) and plan["grad_shs"] < P * 48
    assert d["dumped_outputs"]["grad_shs"] == {"shape": [P, 16, 3], "written": plan["grad_shs"], "sampled": True}
    for n in ("grad_means3D", "grad_opacities", "grad_shs"):
        assert np.any(got[n] != 0), n
    # the same frame from the same arguments in this process
    dev = torch.device("cuda:0")
    s, inp, gcol, ginv = bench.make_inputs(P, W, H, 3, seed=0, device=dev)
    _, raster = bench.rasterizer_for(s, W, H, 3, dev)
    kept = {}
    bench.fwd_bwd_step(raster, inp, gcol, ginv, keep=kept)()
    torch.cuda.synchronize()
    assert np.array_equal(got["radii"], kept["radii"].cpu().numpy().astype(np.float32))
    assert np.abs(got["color"] - kept["color"].detach().cpu().numpy()).max() <= 1e-5
    ref = inp["shs"].grad.cpu().numpy().reshape(-1)[bench.dump_sample("grad_shs", P * 48, plan["grad_shs"])]
    assert np.linalg.norm(got["grad_shs"] - ref) <= 1e-4 * np.linalg.norm(ref)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_rccl_process_group_single_rank():
    """The collective path of the driver's multi-GPU runs on the one-GPU box: bench.py under
    torch.distributed.run with GSR_BENCH_FORCE_PG=1 initialises the RCCL ("nccl") process group
    for its one rank and times through its barriers and all-reduce (RCCL refuses two ranks on one
    device, so N > 1 cannot run here)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT", "LOCAL_WORLD_SIZE", "GSR_BENCH_SHARE_GPU")}
    env["GSR_BENCH_FORCE_PG"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr",
           "127.0.0.1", "--master-port", "29517", os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--gaussians", "200000", "--profile-steps", "1", "--metric-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, env=env, cwd=REPO)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["process_group"] == "nccl"
