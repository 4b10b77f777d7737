"""Cost of preparing a chunk's LiDAR cloud on one GPU, stage by stage.

A synthetic street block: a ground strip and two facades meshed with jittered triangles of 0.2-0.5 m,
four 50 m triangles under the block (a vis2mesh ground plane has such), and a survey of `--points`
points in scan order -- sweep after sweep across the street's profile as the scanner moves along it,
so neighbours in the array are neighbours in space -- 70% within 3 cm of a surface, the rest up to 1 m
off it (what the filter is there to drop).

  1. index:  MeshIndex over the mesh; wall clock per build after a warm-up, and what the index holds
  2. mask:   crop + mesh filter, one kernel (gsr_mesh_near_mask); device events
  3. voxel:  the voxel mean of the kept points at 2000 points per cubic metre (gsr_voxel_mean); wall
             clock (the call synchronises twice for its counts)
For each stage: points per second and the bytes the stage cannot avoid moving (its inputs read once,
its outputs written once) against the time it took.  --cpu N also runs the same rule on the host
over N consecutive survey points from the middle of the street -- scipy's cKDTree over the
triangles' centroids for the candidates, the float64 distance of tests/lidar_ref.py on the candidate
pairs, numpy's voxel mean -- as the CPU baseline, and counts the points on which the two masks differ.

    python tools/lidar_prep_bench.py [--points 20000000] [--length 100] [--pitch 0.35] [--cpu 100000]

Prints one JSON line."""
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

WIDTH, HEIGHT = 24.0, 12.0  # the street's ground strip and its facades, metres


def street_mesh(length, pitch, seed=0):
    """(vertices, faces): three jittered sheets -- ground z = 0, facades y = 0 and y = WIDTH -- and four
    50 m triangles 2 m under the ground."""
    rng = np.random.default_rng(seed)
    vs, fs, base = [], [], 0

    def sheet(nu, nv, to_xyz):
        nonlocal base
        gu, gv = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="ij")
        u = (gu + rng.uniform(-0.22, 0.22, gu.shape)) * pitch
        v = (gv + rng.uniform(-0.22, 0.22, gv.shape)) * pitch
        w = rng.uniform(-0.02, 0.02, gu.shape)
        vs.append(to_xyz(u.reshape(-1), v.reshape(-1), w.reshape(-1)))
        i = (gu[:-1, :-1] * (nv + 1) + gv[:-1, :-1]).reshape(-1) + base
        fs.append(np.concatenate([np.stack([i, i + nv + 1, i + 1], 1), np.stack([i + 1, i + nv + 1, i + nv + 2], 1)]))
        base += (nu + 1) * (nv + 1)

    nx, ny, nz = int(length / pitch), int(WIDTH / pitch), int(HEIGHT / pitch)
    sheet(nx, ny, lambda u, v, w: np.stack([u, v, w], 1))
    sheet(nx, nz, lambda u, v, w: np.stack([u, w, v], 1))
    sheet(nx, nz, lambda u, v, w: np.stack([u, WIDTH + w, v], 1))
    big = np.array([[0, 0, -2], [50, 0, -2], [0, WIDTH, -2], [50, WIDTH, -2], [100, 0, -2], [100, WIDTH, -2]], np.float64)
    big[:, 0] *= length / 100.0
    vs.append(big)
    fs.append(np.array([[0, 1, 2], [2, 1, 3], [1, 4, 3], [3, 4, 5]]) + base)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def street_survey(n, length, device, seed=0, per_sweep=2000):
    """n points in scan order: sweep k covers the profile facade-ground-facade at x = length k / sweeps."""
    g = torch.Generator(device=device).manual_seed(seed)
    i = torch.arange(n, device=device, dtype=torch.float64)
    x = (i / n * length).float() + torch.randn(n, generator=g, device=device) * 0.02
    t = ((i % per_sweep) / per_sweep).float() * (2 * HEIGHT + WIDTH)  # arc length along the profile
    on_left, on_right = t < HEIGHT, t >= HEIGHT + WIDTH
    y = torch.where(on_left, torch.zeros_like(t), torch.where(on_right, torch.full_like(t, WIDTH), t - HEIGHT))
    z = torch.where(on_left, HEIGHT - t, torch.where(on_right, t - HEIGHT - WIDTH, torch.zeros_like(t)))
    off = torch.randn(n, generator=g, device=device) * 0.015
    loose = torch.rand(n, generator=g, device=device) < 0.3
    off = torch.where(loose, 0.1 + 0.9 * torch.rand(n, generator=g, device=device), off)
    inward = torch.where(on_left, 1.0, torch.where(on_right, -1.0, 0.0))
    y = y + inward * off
    z = z + torch.where(on_left | on_right, torch.zeros_like(off), off)
    pts = torch.stack([x, y, z], 1).contiguous()
    col = torch.rand((n, 3), generator=g, device=device)
    return pts, col


def med(v):
    return round(statistics.median(v), 3)


def cpu_baseline(pts, col, vertices, faces, bounds, max_distance, voxel_size):
    """The same rule on the host: cKDTree candidates, float64 distances on the pairs, numpy voxel mean."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import lidar_ref as R
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    crop = R.crop_mask(pts, bounds) & np.isfinite(pts).all(1)
    tri = vertices[faces].astype(np.float64)
    cen = tri.mean(1)
    rad = np.sqrt(((tri - cen[:, None]) ** 2).sum(-1)).max(1)
    small = rad < 1.0
    tree = cKDTree(cen[small])
    ids = np.nonzero(small)[0]
    rows = np.nonzero(crop)[0]
    near = np.zeros(len(pts), bool)
    lists = tree.query_ball_point(pts[rows].astype(np.float64), max_distance + rad[small].max())
    pi = np.repeat(rows, [len(l) for l in lists])
    ti = ids[np.concatenate([np.asarray(l, np.int64) for l in lists])] if len(pi) else np.zeros(0, np.int64)
    for s in range(0, len(pi), 1 << 20):
        p, t = pi[s:s + (1 << 20)], ti[s:s + (1 << 20)]
        d2, _, _ = R.pair_d2(pts[p], vertices[faces[t, 0]], vertices[faces[t, 1]], vertices[faces[t, 2]], np.float64)
        near[p[np.sqrt(d2) <= max_distance]] = True
    for t in np.nonzero(~small)[0]:  # the few large triangles: every point against each
        d2, _, _ = R.pair_d2(pts[rows], vertices[faces[t, 0]][None], vertices[faces[t, 1]][None],
                             vertices[faces[t, 2]][None], np.float64)
        near[rows[np.sqrt(d2) <= max_distance]] = True
    t1 = time.perf_counter()
    means, _, counts, _ = R.voxel_mean(pts[near], col[near], voxel_size)
    t2 = time.perf_counter()
    return near, len(counts), (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(len(pi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--length", type=float, default=100.0)
    ap.add_argument("--pitch", type=float, default=0.35)
    ap.add_argument("--max-distance", type=float, default=0.1)
    ap.add_argument("--density", type=float, default=2000.0)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu", type=int, default=0, help="also run the host baseline on N consecutive points")
    a = ap.parse_args()
    from gs_train import lidar
    dev = torch.device("cuda")
    vertices, faces = street_mesh(a.length, a.pitch)
    pts, col = street_survey(a.points, a.length, dev)
    center, extent = (a.length / 2, WIDTH / 2, 0.0), (a.length * 0.9, WIDTH * 1.2, 100.0)
    box = lidar.crop_bounds(center, extent)
    voxel_size = (1.0 / a.density) ** (1 / 3)
    out = {"points": a.points, "vertices": len(vertices), "triangles": len(faces), "max_distance": a.max_distance,
           "voxel_size": round(voxel_size, 5), "device": torch.cuda.get_device_name(0)}

    # 1. the index
    v_d, f_d = torch.tensor(vertices, device=dev), torch.tensor(faces, device=dev)
    times = []
    for k in range(a.builds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = lidar.MeshIndex(v_d, f_d, max_distance=a.max_distance)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        if k < a.builds:
            index.close()
    info = index.info()
    out["index"] = {"build_ms": [round(t, 2) for t in times[1:]], "build_ms_median": med(times[1:]),
                    "triangles_per_s": round(len(faces) / (statistics.median(times[1:]) * 1e-3)),
                    "bytes": info["bytes"], "cells": info["cells"], "grid": info["grid"],
                    "references": info["references"], "references_per_triangle": round(info["references"] / len(faces), 2),
                    "references_per_cell": round(info["references"] / max(info["cells"], 1), 2),
                    "oversize": info["oversize"],
                    "bytes_min": 12 * len(vertices) + 12 * len(faces) + info["bytes"]}
    out["index"]["GBps_of_min"] = round(out["index"]["bytes_min"] / (out["index"]["build_ms_median"] * 1e-3) / 1e9, 2)

    # 2. crop + mesh filter
    ms = []
    for rep in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        keep = index.near_mask(pts, box=box)
        e1.record()
        e1.synchronize()
        if rep >= 2:
            ms.append(e0.elapsed_time(e1))
    crop_only = lidar._near_mask(pts, None, a.max_distance, box)
    m = statistics.median(ms)
    out["mask"] = {"ms_median": med(ms), "ms_min": round(min(ms), 3), "points_per_s": round(a.points / (m * 1e-3)),
                   "in_box": int(crop_only.sum()), "kept": int(keep.sum()),
                   "bytes_min": 13 * a.points, "GBps_of_min": round(13 * a.points / (m * 1e-3) / 1e9, 1)}

    # 3. the voxel mean of the kept points
    kept, kept_col = pts[keep], col[keep]
    K = kept.shape[0]
    ms = []
    for rep in range(a.reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xyz, rgb, cnt = lidar.voxel_downsample(kept, kept_col, voxel_size)
        torch.cuda.synchronize()
        if rep >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    m = statistics.median(ms)
    M = xyz.shape[0]
    out["voxel"] = {"ms_median": med(ms), "ms_min": round(min(ms), 3), "points_in": K, "voxels_out": M,
                    "points_per_s": round(K / (m * 1e-3)), "largest_voxel": int(cnt.max()) if M else 0,
                    "bytes_min": 24 * K + 28 * M, "GBps_of_min": round((24 * K + 28 * M) / (m * 1e-3) / 1e9, 1),
                    "scratch_bytes": int(lidar.lib().gsr_voxel_mean_scratch_bytes(K))}

    # the three together, as a caller runs them (the compaction of the kept rows included)
    ms = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cc = lidar.prepare_chunk_cloud(pts, col, center, extent, mesh=index, max_distance=a.max_distance,
                                       density=a.density)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["prepare_chunk_cloud_ms"] = [round(t, 2) for t in ms]
    assert cc.points.shape[0] == K and cc.init_points.shape[0] == M

    if a.cpu > 0:
        n = min(a.cpu, a.points)
        s0 = (a.points - n) // 2  # a slice of consecutive sweeps from the middle of the street
        near, voxels, ms_mask, ms_voxel, pairs = cpu_baseline(pts[s0:s0 + n].cpu().numpy(), col[s0:s0 + n].cpu().numpy(),
                                                              vertices, faces, box, a.max_distance, voxel_size)
        gpu = keep[s0:s0 + n].cpu().numpy()
        out["cpu"] = {"points": n, "first": s0, "mask_ms": round(ms_mask, 1), "mask_points_per_s": round(n / (ms_mask * 1e-3)),
                      "candidate_pairs": pairs, "kept": int(near.sum()), "voxel_ms": round(ms_voxel, 1),
                      "voxel_points_per_s": round(int(near.sum()) / max(ms_voxel * 1e-3, 1e-9)), "voxels": voxels,
                      "mask_differs_from_gpu": int((near != gpu).sum())}
    index.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
