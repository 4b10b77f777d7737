"""Cost of the model construction from a cloud and of the scaffold merge (gs_train.model_init,
DESIGN.md section 21) on one GPU, beside the torch-operation formulation of the same lines
(scene/gaussian_model.py:178-264 as gs_train.chunk.street_chunk writes them out), the two alternating
in time.  Each is repeated and the first repetition left out; every figure is between two HIP events
on the stream.

  init     create_from_pcd without a scaffold: N cloud points + S skybox rows, M = 4.  The kNN
           (gsr_knn_mean_dist2 over the S + N rows, the same kernel on both sides) is also timed
           alone, so the part around it shows.
  merge    a scaffold of Ps rows in front of a chunk of Pc rows, M = 16
  coarse   one CoarseTrainStep iteration at the coarse_debug shape of DESIGN.md 7.4c
           (500k rows, SH degree 1, 1080p)

    python tools/model_init_bench.py [--points 1000000 5000000] [--skybox 100000] [--scaffold 1000000]
                                     [--chunk 300000] [--coarse-rows 500000] [--reps 5]

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))

import torch  # noqa: E402

C0 = 0.28209479177387814


def med(v):
    return round(statistics.median(v), 3)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(legs, reps):
    """legs: {name: callable}; each run reps + 1 times, the legs alternating, the first round left out."""
    ms = {k: [] for k in legs}
    for r in range(reps + 1):
        for k, fn in legs.items():
            t, out = timed(fn)
            del out
            if r:
                ms[k].append(t)
    return {k: {"ms": [round(t, 3) for t in v], "ms_median": med(v)} for k, v in ms.items()}


def street_cloud(N, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, device=dev)
    side = N // 2
    road = torch.stack([(u(N - side) * 2 - 1) * 7.0, 1.6 + 0.02 * u(N - side), 200.0 * u(N - side)], 1)
    wall = torch.stack([torch.where(u(side) < 0.5, -7.0, 7.0) + 0.05 * u(side), 1.6 - 8.0 * u(side), 200.0 * u(side)], 1)
    return torch.cat([road, wall]).contiguous(), u(N, 3).contiguous()


def torch_init(pts, col, u_theta, u_phi, M):
    """scene/gaussian_model.py:178-222 in torch operations (skybox mode)."""
    from simple_knn._C import distCUDA2
    S = u_theta.shape[0]
    lo, hi = pts.min(0).values, pts.max(0).values
    mean = 0.5 * (lo + hi)
    radius = torch.linalg.norm(hi - mean)
    theta = 2.0 * math.pi * u_theta
    phi = torch.arccos(1.0 - 1.4 * u_phi)
    sky = torch.stack([radius * 10 * torch.cos(theta) * torch.sin(phi), radius * 10 * torch.sin(theta) * torch.sin(phi),
                       radius * 10 * torch.cos(phi)], 1) + mean
    xyz = torch.cat([sky, pts])
    rgb = torch.cat([torch.ones(S, 3, device=pts.device) * torch.tensor([0.7, 0.8, 0.95], device=pts.device), col])
    feat = torch.zeros(xyz.shape[0], M, 3, device=pts.device)
    feat[:, 0] = (rgb - 0.5) / C0
    d = torch.clamp_min(distCUDA2(xyz), 0.0000001)
    d[:S] *= 10
    d[S:] = torch.clamp_max(d[S:], 10)
    scales = torch.log(torch.sqrt(d))[..., None].repeat(1, 3)
    rots = torch.zeros(xyz.shape[0], 4, device=pts.device)
    rots[:, 0] = 1
    op = torch.full((xyz.shape[0], 1), math.log(0.02 / 0.98), device=pts.device)
    op[:S] = 0.7
    return xyz, feat, op, scales, rots


def torch_merge(sc, S, center, extent, chunk):
    """:248-264 in torch operations."""
    dev = sc.xyz.device
    d1 = torch.abs(sc.xyz - torch.tensor(center, device=dev))
    m = torch.max(d1[:, 0], d1[:, 1])
    sel = torch.logical_and(m > 0.5 * extent[0], m < 1.5 * extent[0])
    sel[:S] = True
    K = sel.nonzero().size(0)
    filler = torch.zeros(K, 16, 3, device=dev)
    filler[:, :4] = sc.shs[sel]
    return (torch.cat([sc.xyz[sel], chunk[0]]), torch.cat([filler, chunk[1]]), torch.cat([sc.opacity_raw[sel], chunk[2]]),
            torch.cat([sc.log_scales[sel], chunk[3]]), torch.cat([sc.rotations[sel], chunk[4]])), K


def bench_init(N, S, reps, dev):
    from gs_train.model_init import init_cloud
    from simple_knn._C import distCUDA2
    pts, col = street_cloud(N, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    u_theta, u_phi = torch.rand(S, generator=g, device=dev), torch.rand(S, generator=g, device=dev)
    xyz = torch_init(pts, col, u_theta, u_phi, 4)[0]
    out = alternate({"kernels": lambda: init_cloud(pts, col, u_theta, u_phi, 4),
                     "torch_ops": lambda: torch_init(pts, col, u_theta, u_phi, 4),
                     "knn_alone": lambda: distCUDA2(xyz)}, reps)
    out.update(points=N, skybox=S, M=4)
    for k in ("kernels", "torch_ops"):
        out[k]["ms_median_less_knn"] = round(out[k]["ms_median"] - out["knn_alone"]["ms_median"], 3)
    return out


def bench_merge(Ps, Pc, reps, dev):
    from gs_train.model_init import scaffold_merge
    from gs_train.scaffold import Scaffold
    g = torch.Generator(device=dev).manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    S = Ps // 10
    xyz = r(Ps, 3) * torch.tensor([60.0, 60.0, 5.0], device=dev)
    sc = Scaffold(xyz.contiguous(), r(Ps, 4, 3), r(Ps, 1), r(Ps, 3), r(Ps, 4), S)
    chunk = (r(Pc, 3), r(Pc, 16, 3), r(Pc, 1), r(Pc, 3), r(Pc, 4))
    center, extent = [3.0, -2.0, 0.0], [50.0, 50.0, 10.0]
    K = scaffold_merge(sc, center, extent, chunk)[1]
    assert K == torch_merge(sc, S, center, extent, chunk)[1]
    out = alternate({"kernels": lambda: scaffold_merge(sc, center, extent, chunk),
                     "torch_ops": lambda: torch_merge(sc, S, center, extent, chunk)}, reps)
    out.update(scaffold_rows=Ps, skybox=S, selected=K, chunk_rows=Pc, M=16)
    return out


def bench_coarse(P, reps, dev):
    from gs_train.coarse import CoarseTrainStep
    from gs_train.harness import make_problem
    torch.manual_seed(0)
    W, H = 1920, 1080
    ts = make_problem(P, W, H, n_views=3, seed=0, sh_degree=1, step_cls=CoarseTrainStep, depth=False, skybox_points=0)
    for _ in range(5):
        ts.step()
    ms = [timed(ts.step)[0] for _ in range(max(reps, 10))]
    return {"rows": P, "width": W, "height": H, "sh_degree": 1, "step_ms": [round(t, 3) for t in ms],
            "step_ms_median": med(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--skybox", type=int, default=100_000)
    ap.add_argument("--scaffold", type=int, default=1_000_000, help="scaffold rows of the merge (0: skip it)")
    ap.add_argument("--chunk", type=int, default=300_000)
    ap.add_argument("--coarse-rows", type=int, default=500_000, help="rows of the coarse iteration (0: skip it)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {}
    for N in a.points:
        out[f"init_{N}"] = bench_init(N, a.skybox, a.reps, dev)
        torch.cuda.empty_cache()
    if a.scaffold:
        out["merge"] = bench_merge(a.scaffold, a.chunk, a.reps, dev)
        torch.cuda.empty_cache()
    if a.coarse_rows:
        out["coarse_step"] = bench_coarse(a.coarse_rows, a.reps, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
