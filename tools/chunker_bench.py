"""Cost of partitioning a calibrated scene into chunks on one GPU, stage by stage.

A synthetic calibration: `--cameras` cameras on a random walk (5 m a step, reflected at the walls of a
square `--side` metres wide), `--points` sparse points in clusters of points / cameras around the
cameras (sigma 30 m), each camera observing `--obs` ids drawn from its own cluster and its two
neighbours' in time (10% of them -1, as COLMAP's unmatched keypoints), errors uniform in [0, 12) so one
point in six is outside C, ids a random permutation with gaps.  chunk_size = side / 10 minus the
padding, which gives a 10 x 10 grid.

  1. each stage of gs_train.chunker.partition_scene between device synchronisations (the module's
     stage timer): classify_points, classify_centers, id_table, camera_counts, candidates, host_draws,
     obs_filter, points_by_cell; wall clock, median of --reps after a warm-up
  2. the whole call, wall clock, inputs already on the device
  3. --cpu-cameras K: the same rule vectorised in numpy on this host (one pass: searchsorted on the
     bounds, a dense id table, bincount per (camera, cell)) over all the points and the first K cameras,
     for scale; its counts are compared with the device's

    python tools/chunker_bench.py [--cameras 20000] [--obs 3000] [--points 20000000] [--cpu-cameras 2000]
                                  [--out profiles/r18_chunker_bench.json]

Prints one JSON line (and writes it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic(cameras, obs, points, side, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    step = torch.randn((cameras, 2), generator=g, device=dev, dtype=torch.float64) * 5.0
    walk = torch.cumsum(step, 0) + side / 2
    walk = torch.abs(torch.remainder(walk, 2 * side) - side)  # reflected into [0, side]
    cam = torch.cat([walk, torch.full((cameras, 1), 2.0, device=dev, dtype=torch.float64)], 1).float()
    per = max(points // cameras, 1)
    owner = torch.clamp(torch.arange(points, device=dev) // per, max=cameras - 1)
    xyz = torch.randn((points, 3), generator=g, device=dev, dtype=torch.float64) * torch.tensor([30.0, 30.0, 5.0], device=dev,
                                                                                              dtype=torch.float64)
    xyz[:, :2] += walk[owner]
    err = torch.rand(points, generator=g, device=dev) * 12.0
    ids = (torch.randperm(points, generator=g, device=dev) * 5) // 4  # unique, with gaps
    rows = (torch.arange(cameras, device=dev)[:, None] - 1) * per + torch.randint(0, 3 * per, (cameras, obs), generator=g,
                                                                                  device=dev)
    rows = torch.clamp(rows, 0, points - 1).reshape(-1)
    obs_id = ids[rows]
    obs_id[torch.rand(rows.shape[0], generator=g, device=dev) < 0.1] = -1
    ptr = torch.arange(cameras + 1, dtype=torch.int64) * obs
    depth = (walk[::4] + 1.0)
    depth = torch.cat([depth, torch.full((depth.shape[0], 1), 2.0, device=dev, dtype=torch.float64)], 1)
    return cam.cpu().numpy(), ptr.numpy(), obs_id, ids, xyz, err, depth.cpu().numpy()


def numpy_rule(cam, ptr, obs_id, ids, xyz, err, bbox, n_w, n_h, cs, K):
    """n_pts, blend, total of the first K cameras and cell32 / cell64 of every point, one vectorised pass."""
    x0, y0 = float(bbox[0, 0]), float(bbox[0, 1])
    bx = np.array([x0 + i * cs for i in range(n_w + 1)])
    by = np.array([y0 + j * cs for j in range(n_h + 1)])
    bx[0], bx[-1], by[0], by[-1] = -1e12, 1e12, -1e12, 1e12

    def cell(p):
        i = np.searchsorted(bx, p[:, 0], side="left") - 1
        j = np.searchsorted(by, p[:, 1], side="left") - 1
        ok = (i >= 0) & (i < n_w) & (j >= 0) & (j < n_h)
        ic, jc = np.clip(i, 0, n_w - 1), np.clip(j, 0, n_h - 1)
        ok &= (bx[ic] < p[:, 0]) & (p[:, 0] < bx[ic + 1]) & (by[jc] < p[:, 1]) & (p[:, 1] < by[jc + 1])
        ok &= (p[:, 2] > -1e12) & (p[:, 2] < 1e12)
        return np.where(ok, ic * n_h + jc, -1).astype(np.int32)

    inC = err < np.float32(10)
    p32 = xyz.astype(np.float32)
    cell64 = cell(xyz)
    cell32 = np.where(inC, cell(p32.astype(np.float64)), -2).astype(np.int32)
    table = np.full(int(ids.max()) + 1, -1, np.int32)
    table[ids] = np.arange(len(ids), dtype=np.int32)
    q = obs_id[:ptr[K]]
    owner = np.repeat(np.arange(K), np.diff(ptr[:K + 1]))
    ok = (q >= 0) & (q < len(table))
    r = np.where(ok, table[np.where(ok, q, 0)], -1)
    c = np.where(r >= 0, cell32[np.maximum(r, 0)], -2)
    vis = (c != -2) & (p32[np.maximum(r, 0)] != 0).any(1)
    cells = n_w * n_h
    has = c >= 0
    blend = np.bincount(owner[has] * cells + c[has], minlength=K * cells).reshape(K, cells)
    hv = has & vis
    n_pts = np.bincount(owner[hv] * cells + c[hv], minlength=K * cells).reshape(K, cells)
    total = np.bincount(owner[vis], minlength=K)
    return cell32, cell64, n_pts, blend, total


def med(v):
    return round(statistics.median(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=20_000)
    ap.add_argument("--obs", type=int, default=3000)
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--side", type=float, default=950.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-cameras", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gs_train import chunker
    dev = torch.device("cuda")
    cs = 100.0
    cam, ptr, obs_id, ids, xyz, err, depth = synthetic(a.cameras, a.obs, a.points, a.side, dev)
    bbox, n_w, n_h = chunker.chunk_grid(cam, cs, 0.2)
    out = {"cameras": a.cameras, "observations": int(obs_id.shape[0]), "points": a.points, "depth_cameras": len(depth),
           "grid": [n_w, n_h], "chunk_size": cs, "device": torch.cuda.get_device_name(0)}

    def run():
        return chunker.partition_scene(cam, ptr, obs_id, ids, xyz, err, depth_centers=depth, chunk_size=cs, device=dev)

    part = run()  # warm-up
    chunker._STAGE_TIMES = {}
    for _ in range(a.reps):
        part = run()
    stages, chunker._STAGE_TIMES = chunker._STAGE_TIMES, None
    out["stage_ms_median"] = {k: med(v) for k, v in stages.items()}
    out["stage_ms_min"] = {k: round(min(v), 3) for k, v in stages.items()}
    ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        part = run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["partition_scene_ms"] = [round(t, 2) for t in ms]
    out["partition_scene_ms_median"] = med(ms)
    out["candidates"] = int(len(part.candidates))
    out["chunks"] = len(part.chunks)
    out["chunk_cameras"] = int(sum(len(c.cameras) for c in part.chunks))
    out["kept_observations"] = int(sum(c.obs_index.shape[0] for c in part.chunks))
    out["chunk_points"] = int(sum(c.points.shape[0] for c in part.chunks))
    out["points_in_C"] = int((part.cell32 != chunker.NOT_IN_C).sum())
    out["cell32_differs_from_cell64"] = int(((part.cell32 != part.cell64) & (part.cell32 != chunker.NOT_IN_C)).sum())
    # the bytes the two large stages cannot avoid: inputs read once, outputs written once
    N, O, M, cells = a.points, int(obs_id.shape[0]), a.cameras, n_w * n_h
    for name, b in (("classify_points", 28 * N + 8 * N), ("camera_counts", 8 * O + 8 * M * cells + 4 * M)):
        out.setdefault("GBps_of_min", {})[name] = round(b / (statistics.median(stages[name]) * 1e-3) / 1e9, 1)

    if a.cpu_cameras > 0:
        K = min(a.cpu_cameras, a.cameras)
        h = [t.cpu().numpy() for t in (obs_id, ids, xyz, err)]
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            cell32, cell64, n_pts, blend, total = numpy_rule(cam, ptr, h[0], h[1], h[2], h[3], bbox, n_w, n_h, cs, K)
        t1 = time.perf_counter()
        out["numpy"] = {"cameras": K, "observations": int(ptr[K]), "points": a.points, "ms": round((t1 - t0) * 1e3, 1),
                        "covers": "cell32, cell64, id table, n_pts, blend, total of these cameras (no candidate list, "
                                  "observation filter or points by cell)",
                        "differs_from_gpu": int((cell32 != part.cell32.cpu().numpy()).sum()
                                                + (cell64 != part.cell64.cpu().numpy()).sum()
                                                + (n_pts != part.n_pts[:K].cpu().numpy()).sum()
                                                + (blend != part.blend[:K].cpu().numpy()).sum()
                                                + (total != part.total[:K].cpu().numpy()).sum())}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
